"""IVFFlatInt8 reports which form of the list scan its last search took (lb_gpu_ivf_last_route), as IVFFlat does; no GPU needed."""
from longbow_amd import ivf


def test_the_int8_handle_has_last_route():
    assert callable(ivf.IVFFlatInt8.last_route)
