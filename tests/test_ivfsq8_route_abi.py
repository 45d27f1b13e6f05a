"""lb_gpu_ivfsq8_last_route: declared in include/longbow_gpu.h, exported, bound in _lib.SIGNATURES, 0 for no handle, and read by
ivfsq8.IVFSQ8.last_route.  All of it runs on a box without a GPU; the routes themselves are in tests/test_gpu_ivfsq8_tile.py."""
import ctypes as C

from tests.test_abi import _declared_symbols

NAME = "lb_gpu_ivfsq8_last_route"


def test_last_route_is_declared_exported_and_bound():
    from longbow_amd import _lib, ivfsq8
    assert NAME in _declared_symbols()
    assert [(s[1], s[2]) for s in _lib.SIGNATURES if s[0] == NAME] == [(C.c_int, [C.c_void_p])]
    assert getattr(_lib.load(), NAME)(None) == 0
    assert callable(ivfsq8.IVFSQ8.last_route)
