"""ivf.IVFFlatUint8 tells the scan form of its last search (lb_gpu_ivf_last_route), as the float32 and int8 handles do."""


def test_the_uint8_handle_has_last_route():
    from longbow_amd import ivf
    assert callable(getattr(ivf.IVFFlatUint8, "last_route", None))
