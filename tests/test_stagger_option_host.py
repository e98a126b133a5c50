"""HM_OPT_GEMM_STAGGER takes 0 (each kernel's default), 1 (lockstep), 2 (staggered), 3 / 4 (one kernel staggered: tuning) and
nothing else: an unknown value is refused instead of silently meaning lockstep."""
from hamer_yolo_amd import lib as L


def test_stagger_option_refuses_unknown_values():
    lib = L.load()
    for v in (1, 2, 3, 4):
        with L.option(L.HM_OPT_GEMM_STAGGER, v):
            assert lib.hm_get_option(L.HM_OPT_GEMM_STAGGER) == v
        assert lib.hm_get_option(L.HM_OPT_GEMM_STAGGER) == 0
    for v in (5, 16, -1):
        assert lib.hm_set_option(L.HM_OPT_GEMM_STAGGER, v) != 0
        assert lib.hm_get_option(L.HM_OPT_GEMM_STAGGER) == 0
