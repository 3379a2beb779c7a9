"""conv_res64pp's ablation modes (no halo DMA / no MFMA / no epilogue: garbage
results) exist only in the diagnostic build: the product library has no
"res64_abl" option, and res64_pp keeps its three values."""
import ctypes

from semanticsegmentation_tensorflow_amd import _lib


def test_product_library_has_no_res64_ablation():
    lib = _lib.load()
    EINVAL = 1
    for v in (0, 1, 5):
        assert lib.seg_set_option(b"res64_abl", v) == EINVAL
    got = ctypes.c_int(-1)
    assert lib.seg_get_option(b"res64_abl", ctypes.byref(got)) == EINVAL
    assert lib.seg_get_option(b"res64_pp", ctypes.byref(got)) == 0 and got.value == 1
    assert lib.seg_set_option(b"res64_pp", 3) == EINVAL
