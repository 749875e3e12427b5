"""What the pLSI fold-in kernel (csrc/plsi_fold_kernels.hpp, compiled into csrc/plsi.hip) promises, checked on the compiler's output -- no GPU:
every instantiation of plsi_fold_kernel keeps its row in registers through all steps (nothing spilled, no private segment), gathers the rows
of Q with 16-byte loads, stores the folded row with 16-byte stores, and holds no atomic and no compare-and-swap (every sum has a fixed order)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def asm():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("needs hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "plsi.s")
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-S", "--cuda-device-only",
               os.path.join(ROOT, "buffalo_amd", "csrc", "plsi.hip"), "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        return open(out).read()


def _kernels(text, stem):
    """{mangled name: body} of every kernel whose name contains `stem`."""
    out = {}
    for m in re.finditer(r"^(_Z\w*%s\w*):" % stem, text, re.M):
        name = m.group(1)
        out[name] = text[m.end():text.index(".Lfunc_end", m.end())]
    return out


def test_fold_kernels_keep_the_row_in_registers_and_gather_16_bytes(asm):
    kernels = _kernels(asm, "plsi_fold_kernel")
    assert len(kernels) == 12, sorted(kernels)          # G = 8, 16, 32, 64 and 64 x {2, 4} chunks, with and without the loss
    for name, body in kernels.items():
        ins = [l.strip() for l in body.split("\n") if l.strip() and not l.strip().startswith(";")]
        assert not any("atomic" in l or "cmpswap" in l for l in ins), (name, [l for l in ins if "atomic" in l or "cmpswap" in l][:3])
        assert not any(l.startswith("scratch_") for l in ins), name
        loads = [l for l in ins if l.startswith("global_load_")]
        wide = [l for l in loads if l.startswith("global_load_dwordx4")]
        narrow = [l for l in loads if not l.startswith("global_load_dwordx4")]
        # rows of Q and the start row move as dwordx4; the only other loads are the entry's key / value and the work item
        assert len(wide) >= 3 and all(re.match(r"global_load_(dword|dwordx2|dwordx3) ", l) for l in narrow), (name, narrow[:4])
        assert len([l for l in ins if l.startswith("global_store_dwordx4")]) >= 1, name
        assert not any(l.startswith("ds_") and not l.startswith(("ds_bpermute", "ds_swizzle")) for l in ins), name      # no LDS: a row stays in its wave
        meta = re.search(r"\.name:\s+%s\n(.*?)\.wavefront_size" % re.escape(name), asm, re.S).group(1)
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1)) == 0, name
        assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", meta).group(1)) == 0, name
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1)) == 0, name


def test_fold_kernels_are_not_counted_as_half_step_kernels(asm):
    assert not any("plsi_half_step_kernel" in name for name in _kernels(asm, "plsi_fold_kernel"))
