"""lb_gpu_ivf_last_route (include/longbow_gpu.h) on a box without a GPU: bound, and 0 for a null handle."""
import ctypes as C


def test_last_route_is_bound_and_a_null_handle_reports_none():
    from longbow_amd import _lib, build, ivf
    build.build()
    lib = _lib.load()
    bound = {s[0]: (s[1], list(s[2])) for s in _lib.SIGNATURES}
    assert bound["lb_gpu_ivf_last_route"] == (C.c_int, [C.c_void_p])
    assert lib.lb_gpu_ivf_last_route(None) == 0
    assert callable(ivf.IVFFlat.last_route) and callable(ivf.IVFFlatIndex.last_route)
