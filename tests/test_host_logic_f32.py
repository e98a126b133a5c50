"""CPU tests of the fp32 YOLOv7 route's host side: the ABI constant, the entry points that must refuse fp32 arguments before
any launch, the split-K size rule, the public switch and the CLI flag.  No GPU compute is launched here."""
import ctypes as C
import os
import re

from hamer_yolo_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HM_ERR_ARG = -1            # hamer_yolo_amd/csrc/common.h


def _conv(dtype, **kw):
    """A 12x20 map, 256 -> 256, k3: K = 2304 (the 16-bit route cuts it into 4 ranges).  Fake, never dereferenced pointers."""
    a = L.ConvArgs(16, 16, 16, 16, 16, 16, 12, 20, 256, 256, 3, 1, 256, 256, 2304, 1, 0, dtype)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_fp32_dtype_in_header_and_binding():
    hdr = open(os.path.join(ROOT, "include", "hamer_hip.h")).read()
    assert int(re.search(r"\bHM_DTYPE_F32\s*=\s*(\d+)", hdr).group(1)) == 2 == L.HM_DTYPE_F32 == L.HM_OUT_F32
    assert int(re.search(r"#define HM_VERSION (\d+)", hdr).group(1)) == 402 == L.HM_VERSION == L.load().hm_version()


def test_fp32_convolution_is_never_split():
    lib = L.load()
    assert lib.hm_conv_splitk_bytes(C.byref(_conv(L.HM_DTYPE_F32))) == 0
    assert lib.hm_conv_splitk_bytes(C.byref(_conv(L.HM_DTYPE_F16))) == 4 * 16 * 12 * 20 * 256 * 4     # unchanged: 4 ranges


def test_fp32_convolution_rejects_relu_and_residual():
    lib = L.load()
    assert lib.hm_conv2d_nhwc(C.byref(_conv(L.HM_DTYPE_F32, act=2)), None) == HM_ERR_ARG
    assert b"fp32" in lib.hm_last_error_string()
    assert lib.hm_conv2d_nhwc(C.byref(_conv(L.HM_DTYPE_F32, act=2, resid=16, ldr=256)), None) == HM_ERR_ARG
    assert lib.hm_conv2d_nhwc(C.byref(_conv(L.HM_DTYPE_F32, act=1, resid=16, ldr=256)), None) == HM_ERR_ARG
    assert lib.hm_conv2d_nhwc(C.byref(_conv(L.HM_DTYPE_F32, act=1, out_f32=1)), None) == HM_ERR_ARG
    assert lib.hm_conv2d_nhwc(C.byref(_conv(L.HM_DTYPE_F32, Cin=24, ldx=24)), None) == HM_ERR_ARG      # Cin a power of two
    assert lib.hm_conv2d_nhwc(C.byref(_conv(L.HM_DTYPE_F32, X=8)), None) == HM_ERR_ARG                # X 16-byte aligned
    assert lib.hm_conv2d_nhwc(C.byref(_conv(3)), None) == HM_ERR_ARG                                  # unknown dtype


def test_stem_pair_rejects_fp32():
    lib = L.load()
    first = L.ConvArgs(16, 16, 32, 16, 16, 1, 64, 96, 8, 32, 3, 1, 8, 32, 128, 1, 0, L.HM_DTYPE_F32)
    second = L.ConvArgs(32, 16, 48, 16, 16, 1, 64, 96, 32, 64, 3, 2, 32, 64, 320, 1, 0, L.HM_DTYPE_F32)
    assert lib.hm_conv2d_stem_pair(C.byref(first), C.byref(second), None) == HM_ERR_ARG
    assert b"fp32" in lib.hm_last_error_string()


def test_other_entry_points_keep_rejecting_fp32():
    lib = L.load()
    assert lib.hm_nchw3_to_nhwc8(C.c_void_p(16), C.c_void_p(16), 1, 8, 8, L.HM_DTYPE_F32, None) == HM_ERR_ARG
    assert lib.hm_gap_linear(C.c_void_p(16), 64, 512, C.c_void_p(16), C.c_float(0.0), C.c_void_p(16), C.c_void_p(16), 1,
                             L.HM_DTYPE_F32, None) == HM_ERR_ARG


def test_cli_flag_and_config_default():
    from hamer_yolo_amd import d_infer, infer
    from hamer_yolo_amd.config.yolo_config import Config, yolo_opt
    assert Config.precise is False and yolo_opt.precise is False
    a = infer._parser().parse_args(["--input", "i", "--output", "o", "--precise-detector"])
    assert a.precise_detector is True
    assert infer._parser().parse_args(["--input", "i", "--output", "o"]).precise_detector is False
    b = d_infer._parser().parse_args(["--input", "i", "--output", "o", "--intrinsics", "k.txt", "--precise-detector"])
    assert b.precise_detector is True
