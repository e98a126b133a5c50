"""CPU-side audit of the emitted gfx950 ISA of the staggered GEMM kernels (gemm_pxs_kernel, gemm_x3rs_kernel).

They issue the same untracked register-destination loads as their lockstep forms (the bias pair, the residual pieces), in both
roles, so the same property is checked on the emitted code (tools/isa_async_reg_check.py): no instruction touches a destination
register before the hand-counted wait that names it.  And their counted `vmcnt` waits assume that copies, those loads and the
epilogue's stores are the only vector-memory instructions: a lagging wave carries a fragment set across every barrier at
248-254 VGPRs, so "no spill" is pinned here (private segment size 0, no scratch instruction)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.isa_async_reg_check import audit  # noqa: E402

SRC = os.path.join(ROOT, "hamer_yolo_amd", "csrc", "gemm.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

PXS = ["gemm_pxs_kernelI%sLi%dELb%dE" % (t, epi, direct) for t in ("4TF16", "5TBf16") for epi in (0, 1, 4) for direct in (0, 1)]      # HM_EPI_STORE, _GELU, _SILU; through LDS / lane swaps
X3RS = ["gemm_x3rs_kernelI4TF16E", "gemm_x3rs_kernelI5TBf16E"]


@pytest.fixture(scope="module")
def gemm_isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("isa") / "gemm.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only", SRC, "-o", out],
                   check=True, capture_output=True, timeout=900)
    return open(out).read()


def _instantiated(isa, names):
    return [n for n in names if re.search(r"^_Z\w*" + re.escape(n) + r"\w*:", isa, re.M)]


def test_every_staggered_form_is_there(gemm_isa):
    """Every (type, epilogue, form) the launchers can pick has its staggered kernel."""
    assert _instantiated(gemm_isa, X3RS) == X3RS
    assert _instantiated(gemm_isa, PXS) == PXS


@pytest.mark.parametrize("kernel,min_loads", [(k, 2) for k in PXS] + [(k, 32) for k in X3RS])
def test_asm_loaded_registers_are_fenced(gemm_isa, kernel, min_loads):
    ok, report, n = audit(gemm_isa, kernel, "vm")
    assert n >= min_loads, f"{kernel}: expected at least {min_loads} asm-issued register loads, found {n}\n{report}"
    assert ok, report


def test_staggered_kernels_do_not_spill(gemm_isa):
    seen = 0
    for m in re.finditer(r"^(_Z\w*(gemm_pxs|gemm_x3rs)_kernel\w*):(.*?)\.amdhsa_kernel", gemm_isa, re.S | re.M):
        seen += 1
        assert "scratch_" not in m.group(3), m.group(1)
        priv = re.search(re.escape(m.group(1)) + r"\.private_seg_size, (\d+)", gemm_isa)
        assert priv and int(priv.group(1)) == 0, m.group(1)
    assert seen == len(PXS) + len(X3RS), seen
