"""ctypes loader for liblongbow_gpu.so -- the only place the library is opened.

Fails loudly: a missing/unloadable library raises ImportError-like RuntimeError at
first use; a missing GPU raises GPUNotAvailable (the reference's ErrGPUNotAvailable,
internal/gpu/stub.go:10).  Nothing here ever computes on the CPU.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# LB_GPU_SO selects another build of the library (tools/ use the -DLB_DIAG build, liblongbow_gpu_diag.so)
SO_PATH = os.environ.get("LB_GPU_SO") or os.path.join(_HERE, "liblongbow_gpu.so")

LB_OK = 0
STATUS = {0: "ok", 1: "invalid argument", 2: "index is closed", 3: "GPU not available",
          4: "HIP runtime error", 5: "out of device memory", 6: "unsupported configuration",
          7: "internal error", 8: "context canceled", 9: "context deadline exceeded"}


class LongbowGPUError(RuntimeError):
    def __init__(self, code, msg=""):
        self.code = code
        super().__init__(f"longbow_gpu: {STATUS.get(code, 'error')} (code {code}){': ' + msg if msg else ''}")


class GPUNotAvailable(LongbowGPUError):
    """internal/gpu/stub.go:10 ErrGPUNotAvailable"""


class Canceled(LongbowGPUError):
    """context.Canceled: the call's Cancel fired (internal/store/adaptive_index.go:182 returns ctx.Err())"""


class DeadlineExceeded(LongbowGPUError):
    """context.DeadlineExceeded"""


_lib = None

# every symbol include/longbow_gpu.h declares: (name, restype, argtypes)
_vp, _i, _i64, _u64, _sz = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_size_t
_ip = C.POINTER(C.c_int)
SIGNATURES = [
    ("lb_gpu_device_count", _i, []),
    ("lb_gpu_version", C.c_char_p, []),
    ("lb_gpu_status_string", C.c_char_p, [_i]),
    ("lb_gpu_index_new", _vp, [_i, _i, _i, _ip]),
    ("lb_gpu_index_free", None, [_vp]),
    ("lb_gpu_last_error", C.c_char_p, [_vp]),
    ("lb_gpu_index_set_order", _i, [_vp, _i]),
    ("lb_gpu_index_set_candidate_mode", _i, [_vp, _i]),
    ("lb_gpu_index_set_f16_image", _i, [_vp, _i]),
    ("lb_gpu_index_f16_image_bytes", _i64, [_vp]),
    ("lb_gpu_index_set_search_combining", _i, [_vp, _i]),
    ("lb_gpu_index_combining_stats", _i, [_vp, C.POINTER(C.c_int64)]),
    ("lb_gpu_index_ntotal", _i64, [_vp]),
    ("lb_gpu_index_dim", _i, [_vp]),
    ("lb_gpu_index_device", _i, [_vp]),
    ("lb_cancel_new", _vp, []),
    ("lb_cancel_fire", None, [_vp]),
    ("lb_cancel_set_deadline_ms", None, [_vp, _i64]),
    ("lb_cancel_state", _i, [_vp]),
    ("lb_cancel_free", None, [_vp]),
    ("lb_gpu_index_search_ctx", _i, [_vp, _i64, _vp, _i, _vp, _vp, _vp]),
    ("lb_gpu_index_search_device_ctx", _i, [_vp, _i64, _vp, _i, _vp, _vp, _vp, _vp]),
    ("lb_simd_distance_batch", _i, [_i, _i, _i, _vp, _i, _vp, _vp, _i64, _vp]),
    ("lb_gpu_pq_search_ctx", _i, [_vp, _i64, _vp, _i, _vp, _vp, _vp]),
    ("lb_gpu_pq_search_device_ctx", _i, [_vp, _i64, _vp, _i, _vp, _vp, _vp, _vp]),
    ("lb_gpu_pq_set_search_combining", _i, [_vp, _i]),
    ("lb_gpu_pq_combining_stats", _i, [_vp, C.POINTER(C.c_int64)]),
    ("lb_gpu_pq_set_prefilter", _i, [_vp, _i]),
    ("lb_gpu_pq_last_search_stats", _i, [_vp, C.POINTER(C.c_int64)]),
    ("lb_gpu_index_reserve", _i, [_vp, _i64]),
    ("lb_gpu_index_add", _i, [_vp, _i64, _vp, _vp]),
    ("lb_gpu_index_add_device", _i, [_vp, _i64, _vp, _vp]),
    ("lb_gpu_index_search", _i, [_vp, _i64, _vp, _i, _vp, _vp]),
    ("lb_gpu_index_search_device", _i, [_vp, _i64, _vp, _i, _vp, _vp, _vp]),
    ("lb_gpu_index_new_f16", _vp, [_i, _i, _i, _ip]),
    ("lb_gpu_index_dtype", _i, [_vp]),
    ("lb_gpu_index_add_f16", _i, [_vp, _i64, _vp, _vp]),
    ("lb_gpu_index_add_f16_device", _i, [_vp, _i64, _vp, _vp]),
    ("lb_gpu_index_search_f16", _i, [_vp, _i64, _vp, _i, _vp, _vp]),
    ("lb_gpu_index_search_f16_ctx", _i, [_vp, _i64, _vp, _i, _vp, _vp, _vp]),
    ("lb_gpu_index_search_f16_device_ctx", _i, [_vp, _i64, _vp, _i, _vp, _vp, _vp, _vp]),
    ("lb_gpu_index_hbm_bytes", _i64, [_vp]),
    ("lb_gpu_index_new_i8", _vp, [_i, _i, _i, _ip]),
    ("lb_gpu_index_add_i8", _i, [_vp, _i64, _vp, _vp]),
    ("lb_gpu_index_add_i8_device", _i, [_vp, _i64, _vp, _vp]),
    ("lb_gpu_index_search_i8", _i, [_vp, _i64, _vp, _i, _vp, _vp]),
    ("lb_gpu_index_search_i8_ctx", _i, [_vp, _i64, _vp, _i, _vp, _vp, _vp]),
    ("lb_gpu_index_search_i8_device_ctx", _i, [_vp, _i64, _vp, _i, _vp, _vp, _vp, _vp]),
    ("lb_gpu_index_search_bitmap_ctx", _i, [_vp, _i64, _vp, _i, _vp, _i64, _vp, _vp, _vp]),
    ("lb_gpu_index_search_bitmap_device_ctx", _i, [_vp, _i64, _vp, _i, _vp, _i64, _vp, _vp, _vp, _vp]),
    ("lb_gpu_index_search_f16_bitmap_ctx", _i, [_vp, _i64, _vp, _i, _vp, _i64, _vp, _vp, _vp]),
    ("lb_gpu_index_search_f16_bitmap_device_ctx", _i, [_vp, _i64, _vp, _i, _vp, _i64, _vp, _vp, _vp, _vp]),
    ("lb_gpu_index_search_i8_bitmap_ctx", _i, [_vp, _i64, _vp, _i, _vp, _i64, _vp, _vp, _vp]),
    ("lb_gpu_index_search_i8_bitmap_device_ctx", _i, [_vp, _i64, _vp, _i, _vp, _i64, _vp, _vp, _vp, _vp]),
    ("lb_gpu_index_set_filter", _i, [_vp, _vp, _i64]),
    ("lb_gpu_index_nvisible", _i64, [_vp]),
    ("lb_gpu_index_filter_int64", _i, [_vp, _vp, _i64, _i64, _i, _vp, _i64, _i]),
    ("lb_gpu_index_filter_float32", _i, [_vp, _vp, _i64, C.c_float, _i, _vp, _i64, _i]),
    ("lb_gpu_index_remove", _i, [_vp, _i64, _vp, C.POINTER(C.c_int64)]),
    ("lb_gpu_index_remove_device", _i, [_vp, _i64, _vp, C.POINTER(C.c_int64)]),
    ("lb_gpu_index_remove_rows", _i, [_vp, _i64, _vp, C.POINTER(C.c_int64)]),
    ("lb_gpu_index_nlive", _i64, [_vp]),
    ("lb_gpu_index_ndeleted", _i64, [_vp]),
    ("lb_gpu_index_compact", _i, [_vp, _vp, _i64]),
    ("lb_gpu_index_last_fallbacks", _i64, [_vp]),
    ("lb_gpu_index_fused_giveups", _i64, [_vp]),
    ("lb_gpu_index_last_route", _i, [_vp]),
    ("lb_gpu_index_rerank", _i, [_vp, _vp, _vp, _i64, _i, _vp, _vp]),
    ("lb_gpu_index_rerank_device", _i, [_vp, _vp, _vp, _i64, _i, _vp, _vp, _vp]),
    ("lb_gpu_index_refine", _i, [_vp, _i64, _vp, _i64, _vp, _i, _i, _vp, _vp]),
    ("lb_gpu_index_refine_ctx", _i, [_vp, _i64, _vp, _i64, _vp, _i, _i, _vp, _vp, _vp]),
    ("lb_gpu_index_refine_device_ctx", _i, [_vp, _i64, _vp, _i64, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    ("lb_gpu_index_refine_last_timing", _i, [_vp, C.POINTER(C.c_float)]),
    ("lb_simd_match_int64", _i, [_i, _vp, _i64, _i64, _i, _vp]),
    ("lb_simd_match_float32", _i, [_i, _vp, _i64, C.c_float, _i, _vp]),
    ("lb_simd_and_bytes", _i, [_i, _vp, _vp, _i64]),
    ("lb_simd_distance_batch_flat", _i, [_i, _i, _i, _vp, _vp, _i64, _i, _vp]),
    ("lb_simd_distance_batch_flat_device", _i, [_i, _i, _i, _vp, _vp, _i64, _i, _vp, _vp]),
    ("lb_gpu_pq_new", _vp, [_i, _vp, _sz, _ip]),
    ("lb_gpu_pq_free", None, [_vp]),
    ("lb_gpu_pq_last_error", C.c_char_p, [_vp]),
    ("lb_gpu_pq_m", _i, [_vp]),
    ("lb_gpu_pq_dims", _i, [_vp]),
    ("lb_gpu_pq_ntotal", _i64, [_vp]),
    ("lb_gpu_pq_add_codes", _i, [_vp, _i64, _vp]),
    ("lb_gpu_pq_add_codes_device", _i, [_vp, _i64, _vp]),
    ("lb_gpu_pq_reserve", _i, [_vp, _i64]),
    ("lb_gpu_pq_get_codes", _i, [_vp, _i64, _i64, _vp]),
    ("lb_gpu_pq_encode", _i, [_vp, _i64, _vp, _vp]),
    ("lb_gpu_pq_encode_device", _i, [_vp, _i64, _vp, _vp, _vp]),
    ("lb_gpu_pq_add_vectors_device", _i, [_vp, _i64, _vp]),
    ("lb_gpu_pq_decode", _i, [_vp, _i64, _vp, _vp]),
    ("lb_gpu_pq_decode_device", _i, [_vp, _i64, _vp, _vp, _vp]),
    ("lb_gpu_pq_rerank", _i, [_vp, _vp, _vp, _i64, _vp, _vp]),
    ("lb_gpu_pq_rerank_device", _i, [_vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    ("lb_gpu_pq_set_profiling", _i, [_vp, _i]),
    ("lb_gpu_pq_last_timing", _i, [_vp, _vp]),
    ("lb_gpu_pq_build_adc_table", _i, [_vp, _vp, _vp]),
    ("lb_gpu_pq_adc_distance_batch", _i, [_vp, _vp, _i64, _i64, _vp]),
    ("lb_gpu_pq_search", _i, [_vp, _i64, _vp, _i, _vp, _vp]),
    ("lb_gpu_pq_search_device", _i, [_vp, _i64, _vp, _i, _vp, _vp, _vp]),
    ("lb_gpu_pq_set_filter", _i, [_vp, _vp, _i64]),
    ("lb_gpu_pq_filter_int64", _i, [_vp, _vp, _i64, _i64, _i, _vp, _i64, _i]),
    ("lb_gpu_pq_filter_float32", _i, [_vp, _vp, _i64, C.c_float, _i, _vp, _i64, _i]),
    ("lb_gpu_pq_nvisible", _i64, [_vp]),
    ("lb_gpu_pq_train", _i, [_i, _i, _i, _i, _i64, _vp, _i, _u64, _vp, _vp, _sz, _vp, _vp]),
    ("lb_gpu_pq_train_device", _i, [_i, _i, _i, _i, _i64, _vp, _i, _u64, _vp, _vp, _sz, _vp, _vp, _vp]),
    ("lb_gpu_pq_blob_bytes", _sz, [_i, _i, _i]),
    ("lb_gpu_pq_train_last_timing", _i, [_vp]),
    ("lb_gpu_ivf_train", _i, [_i, _i, _i, _i64, _vp, _i, _u64, _vp, _vp, _vp, _vp]),
    ("lb_gpu_ivf_train_device", _i, [_i, _i, _i, _i64, _vp, _i, _u64, _vp, _vp, _vp, _vp, _vp]),
    ("lb_gpu_ivf_train_last_timing", _i, [_vp]),
    ("lb_gpu_bq_new", _vp, [_i, _i, _ip]),
    ("lb_gpu_bq_free", None, [_vp]),
    ("lb_gpu_bq_last_error", C.c_char_p, [_vp]),
    ("lb_gpu_bq_dims", _i, [_vp]),
    ("lb_gpu_bq_words", _i, [_vp]),
    ("lb_gpu_bq_ntotal", _i64, [_vp]),
    ("lb_gpu_bq_reserve", _i, [_vp, _i64]),
    ("lb_gpu_bq_add_codes", _i, [_vp, _i64, _vp]),
    ("lb_gpu_bq_add_codes_device", _i, [_vp, _i64, _vp]),
    ("lb_gpu_bq_get_codes", _i, [_vp, _i64, _i64, _vp]),
    ("lb_gpu_bq_encode", _i, [_vp, _i64, _vp, _vp]),
    ("lb_gpu_bq_encode_device", _i, [_vp, _i64, _vp, _vp, _vp]),
    ("lb_gpu_bq_add_vectors", _i, [_vp, _i64, _vp]),
    ("lb_gpu_bq_add_vectors_device", _i, [_vp, _i64, _vp]),
    ("lb_gpu_bq_decode", _i, [_vp, _i64, _vp, _vp]),
    ("lb_gpu_bq_hamming_batch", _i, [_vp, _vp, _i64, _i64, _vp]),
    ("lb_gpu_bq_rerank", _i, [_vp, _vp, _vp, _i64, _vp, _vp]),
    ("lb_gpu_bq_rerank_device", _i, [_vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    ("lb_gpu_bq_search_codes", _i, [_vp, _i64, _vp, _i, _vp, _vp]),
    ("lb_gpu_bq_search", _i, [_vp, _i64, _vp, _i, _vp, _vp]),
    ("lb_gpu_bq_search_ctx", _i, [_vp, _i64, _vp, _i, _vp, _vp, _vp]),
    ("lb_gpu_bq_search_device_ctx", _i, [_vp, _i64, _vp, _i, _vp, _vp, _vp, _vp]),
    ("lb_gpu_bq_set_filter", _i, [_vp, _vp, _i64]),
    ("lb_gpu_bq_filter_int64", _i, [_vp, _vp, _i64, _i64, _i, _vp, _i64, _i]),
    ("lb_gpu_bq_filter_float32", _i, [_vp, _vp, _i64, C.c_float, _i, _vp, _i64, _i]),
    ("lb_gpu_bq_nvisible", _i64, [_vp]),
    ("lb_gpu_sq8_new", _vp, [_i, _i, _ip]),
    ("lb_gpu_sq8_free", None, [_vp]),
    ("lb_gpu_sq8_last_error", C.c_char_p, [_vp]),
    ("lb_gpu_sq8_dims", _i, [_vp]),
    ("lb_gpu_sq8_ntotal", _i64, [_vp]),
    ("lb_gpu_sq8_reserve", _i, [_vp, _i64]),
    ("lb_gpu_sq8_trained", _i, [_vp]),
    ("lb_gpu_sq8_set_bounds", _i, [_vp, _vp, _vp]),
    ("lb_gpu_sq8_train", _i, [_vp, _i64, _vp]),
    ("lb_gpu_sq8_train_device", _i, [_vp, _i64, _vp]),
    ("lb_gpu_sq8_get_bounds", _i, [_vp, _vp, _vp]),
    ("lb_gpu_sq8_encode", _i, [_vp, _i64, _vp, _vp]),
    ("lb_gpu_sq8_encode_device", _i, [_vp, _i64, _vp, _vp, _vp]),
    ("lb_gpu_sq8_decode", _i, [_vp, _i64, _vp, _vp]),
    ("lb_gpu_sq8_add_codes", _i, [_vp, _i64, _vp]),
    ("lb_gpu_sq8_add_codes_device", _i, [_vp, _i64, _vp]),
    ("lb_gpu_sq8_add_vectors", _i, [_vp, _i64, _vp]),
    ("lb_gpu_sq8_add_vectors_device", _i, [_vp, _i64, _vp]),
    ("lb_gpu_sq8_get_codes", _i, [_vp, _i64, _i64, _vp]),
    ("lb_gpu_sq8_distance_batch", _i, [_vp, _vp, _i64, _i64, _vp]),
    ("lb_gpu_sq8_rerank", _i, [_vp, _vp, _vp, _i64, _vp, _vp]),
    ("lb_gpu_sq8_rerank_device", _i, [_vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    ("lb_gpu_sq8_search_codes", _i, [_vp, _i64, _vp, _i, _vp, _vp]),
    ("lb_gpu_sq8_search", _i, [_vp, _i64, _vp, _i, _vp, _vp]),
    ("lb_gpu_sq8_search_ctx", _i, [_vp, _i64, _vp, _i, _vp, _vp, _vp]),
    ("lb_gpu_sq8_search_device_ctx", _i, [_vp, _i64, _vp, _i, _vp, _vp, _vp, _vp]),
    ("lb_gpu_sq8_set_filter", _i, [_vp, _vp, _i64]),
    ("lb_gpu_sq8_filter_int64", _i, [_vp, _vp, _i64, _i64, _i, _vp, _i64, _i]),
    ("lb_gpu_sq8_filter_float32", _i, [_vp, _vp, _i64, C.c_float, _i, _vp, _i64, _i]),
    ("lb_gpu_sq8_nvisible", _i64, [_vp]),
    ("lb_gpu_ivf_new", _vp, [_i, _i, _i, _i, _i, _vp, _ip]),
    ("lb_gpu_ivf_new_f16", _vp, [_i, _i, _i, _i, _i, _vp, _ip]),
    ("lb_gpu_ivf_dtype", _i, [_vp]),
    ("lb_gpu_ivf_add_f16", _i, [_vp, _i64, _vp, _vp]),
    ("lb_gpu_ivf_add_f16_device", _i, [_vp, _i64, _vp, _vp]),
    ("lb_gpu_ivf_new_i8", _vp, [_i, _i, _i, _i, _i, _vp, _ip]),
    ("lb_gpu_ivf_add_i8", _i, [_vp, _i64, _vp, _vp]),
    ("lb_gpu_ivf_add_i8_device", _i, [_vp, _i64, _vp, _vp]),
    ("lb_gpu_ivf_free", None, [_vp]),
    ("lb_gpu_ivf_last_error", C.c_char_p, [_vp]),
    ("lb_gpu_ivf_dim", _i, [_vp]),
    ("lb_gpu_ivf_metric", _i, [_vp]),
    ("lb_gpu_ivf_order", _i, [_vp]),
    ("lb_gpu_ivf_nlist", _i, [_vp]),
    ("lb_gpu_ivf_ntotal", _i64, [_vp]),
    ("lb_gpu_ivf_hbm_bytes", _i64, [_vp]),
    ("lb_gpu_ivf_get_centroids", _i, [_vp, _vp]),
    ("lb_gpu_ivf_reserve", _i, [_vp, _i64]),
    ("lb_gpu_ivf_add", _i, [_vp, _i64, _vp, _vp]),
    ("lb_gpu_ivf_add_device", _i, [_vp, _i64, _vp, _vp]),
    ("lb_gpu_ivf_list_sizes", _i, [_vp, _vp]),
    ("lb_gpu_ivf_assignments", _i, [_vp, _i64, _i64, _vp]),
    ("lb_gpu_ivf_search", _i, [_vp, _i64, _vp, _i, _i, _vp, _vp]),
    ("lb_gpu_ivf_search_ctx", _i, [_vp, _i64, _vp, _i, _i, _vp, _vp, _vp]),
    ("lb_gpu_ivf_search_device_ctx", _i, [_vp, _i64, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    ("lb_gpu_ivf_search_i8", _i, [_vp, _i64, _vp, _i, _i, _vp, _vp]),
    ("lb_gpu_ivf_search_i8_ctx", _i, [_vp, _i64, _vp, _i, _i, _vp, _vp, _vp]),
    ("lb_gpu_ivf_search_i8_device_ctx", _i, [_vp, _i64, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    ("lb_gpu_ivf_search_bitmap_ctx", _i, [_vp, _i64, _vp, _i, _i, _vp, _i64, _i64, _vp, _vp, _vp]),
    ("lb_gpu_ivf_search_bitmap_device_ctx", _i, [_vp, _i64, _vp, _i, _i, _vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    ("lb_gpu_ivf_search_i8_bitmap_ctx", _i, [_vp, _i64, _vp, _i, _i, _vp, _i64, _i64, _vp, _vp, _vp]),
    ("lb_gpu_ivf_search_i8_bitmap_device_ctx", _i, [_vp, _i64, _vp, _i, _i, _vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    ("lb_gpu_ivf_set_filter", _i, [_vp, _vp, _i64]),
    ("lb_gpu_ivf_filter_int64", _i, [_vp, _vp, _i64, _i64, _i, _vp, _i64, _i]),
    ("lb_gpu_ivf_filter_float32", _i, [_vp, _vp, _i64, C.c_float, _i, _vp, _i64, _i]),
    ("lb_gpu_ivf_nvisible", _i64, [_vp]),
    ("lb_gpu_ivf_last_search_stats", _i, [_vp, C.POINTER(C.c_int64)]),
    ("lb_gpu_ivf_set_profiling", _i, [_vp, _i]),
    ("lb_gpu_ivf_last_timing", _i, [_vp, _vp]),
    ("lb_gpu_ivf_last_build_timing", _i, [_vp, _vp]),
    ("lb_gpu_ivf_remove", _i, [_vp, _i64, _vp, C.POINTER(C.c_int64)]),
    ("lb_gpu_ivf_remove_device", _i, [_vp, _i64, _vp, C.POINTER(C.c_int64)]),
    ("lb_gpu_ivf_remove_rows", _i, [_vp, _i64, _vp, C.POINTER(C.c_int64)]),
    ("lb_gpu_ivf_nlive", _i64, [_vp]),
    ("lb_gpu_ivf_ndeleted", _i64, [_vp]),
    ("lb_gpu_ivf_compact", _i, [_vp, _vp, _i64]),
    ("lb_gpu_ivfpq_new", _vp, [_i, _vp, _sz, _i, _i, _vp, _ip]),
    ("lb_gpu_ivfpq_new_residual", _vp, [_i, _vp, _sz, _i, _i, _vp, _ip]),
    ("lb_gpu_ivfpq_residual", _i, [_vp]),
    ("lb_gpu_ivfpq_free", None, [_vp]),
    ("lb_gpu_ivfpq_last_error", C.c_char_p, [_vp]),
    ("lb_gpu_ivfpq_dims", _i, [_vp]),
    ("lb_gpu_ivfpq_m", _i, [_vp]),
    ("lb_gpu_ivfpq_order", _i, [_vp]),
    ("lb_gpu_ivfpq_nlist", _i, [_vp]),
    ("lb_gpu_ivfpq_ntotal", _i64, [_vp]),
    ("lb_gpu_ivfpq_hbm_bytes", _i64, [_vp]),
    ("lb_gpu_ivfpq_get_centroids", _i, [_vp, _vp]),
    ("lb_gpu_ivfpq_reserve", _i, [_vp, _i64]),
    ("lb_gpu_ivfpq_add", _i, [_vp, _i64, _vp, _vp]),
    ("lb_gpu_ivfpq_add_device", _i, [_vp, _i64, _vp, _vp]),
    ("lb_gpu_ivfpq_get_codes", _i, [_vp, _i64, _i64, _vp]),
    ("lb_gpu_ivfpq_list_sizes", _i, [_vp, _vp]),
    ("lb_gpu_ivfpq_assignments", _i, [_vp, _i64, _i64, _vp]),
    ("lb_gpu_ivfpq_search", _i, [_vp, _i64, _vp, _i, _i, _vp, _vp]),
    ("lb_gpu_ivfpq_search_ctx", _i, [_vp, _i64, _vp, _i, _i, _vp, _vp, _vp]),
    ("lb_gpu_ivfpq_search_device_ctx", _i, [_vp, _i64, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    ("lb_gpu_ivfpq_search_bitmap_ctx", _i, [_vp, _i64, _vp, _i, _i, _vp, _i64, _i64, _vp, _vp, _vp]),
    ("lb_gpu_ivfpq_search_bitmap_device_ctx", _i, [_vp, _i64, _vp, _i, _i, _vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    ("lb_gpu_ivfpq_set_filter", _i, [_vp, _vp, _i64]),
    ("lb_gpu_ivfpq_filter_int64", _i, [_vp, _vp, _i64, _i64, _i, _vp, _i64, _i]),
    ("lb_gpu_ivfpq_filter_float32", _i, [_vp, _vp, _i64, C.c_float, _i, _vp, _i64, _i]),
    ("lb_gpu_ivfpq_nvisible", _i64, [_vp]),
    ("lb_gpu_ivfpq_last_search_stats", _i, [_vp, C.POINTER(C.c_int64)]),
    ("lb_gpu_ivfpq_set_profiling", _i, [_vp, _i]),
    ("lb_gpu_ivfpq_last_timing", _i, [_vp, _vp]),
    ("lb_gpu_ivfpq_last_build_timing", _i, [_vp, _vp]),
    ("lb_gpu_ivfpq_remove", _i, [_vp, _i64, _vp, C.POINTER(C.c_int64)]),
    ("lb_gpu_ivfpq_remove_device", _i, [_vp, _i64, _vp, C.POINTER(C.c_int64)]),
    ("lb_gpu_ivfpq_remove_rows", _i, [_vp, _i64, _vp, C.POINTER(C.c_int64)]),
    ("lb_gpu_ivfpq_nlive", _i64, [_vp]),
    ("lb_gpu_ivfpq_ndeleted", _i64, [_vp]),
    ("lb_gpu_ivfpq_compact", _i, [_vp, _vp, _i64]),
    ("lb_gpu_ivfsq8_new", _vp, [_i, _i, _vp, _vp, _i, _i, _vp, _ip]),
    ("lb_gpu_ivfsq8_free", None, [_vp]),
    ("lb_gpu_ivfsq8_last_error", C.c_char_p, [_vp]),
    ("lb_gpu_ivfsq8_dims", _i, [_vp]),
    ("lb_gpu_ivfsq8_order", _i, [_vp]),
    ("lb_gpu_ivfsq8_nlist", _i, [_vp]),
    ("lb_gpu_ivfsq8_ntotal", _i64, [_vp]),
    ("lb_gpu_ivfsq8_hbm_bytes", _i64, [_vp]),
    ("lb_gpu_ivfsq8_get_bounds", _i, [_vp, _vp, _vp]),
    ("lb_gpu_ivfsq8_get_centroids", _i, [_vp, _vp]),
    ("lb_gpu_ivfsq8_reserve", _i, [_vp, _i64]),
    ("lb_gpu_ivfsq8_add", _i, [_vp, _i64, _vp, _vp]),
    ("lb_gpu_ivfsq8_add_device", _i, [_vp, _i64, _vp, _vp]),
    ("lb_gpu_ivfsq8_get_codes", _i, [_vp, _i64, _i64, _vp]),
    ("lb_gpu_ivfsq8_list_sizes", _i, [_vp, _vp]),
    ("lb_gpu_ivfsq8_assignments", _i, [_vp, _i64, _i64, _vp]),
    ("lb_gpu_ivfsq8_search", _i, [_vp, _i64, _vp, _i, _i, _vp, _vp]),
    ("lb_gpu_ivfsq8_search_ctx", _i, [_vp, _i64, _vp, _i, _i, _vp, _vp, _vp]),
    ("lb_gpu_ivfsq8_search_device_ctx", _i, [_vp, _i64, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    ("lb_gpu_ivfsq8_search_bitmap_ctx", _i, [_vp, _i64, _vp, _i, _i, _vp, _i64, _i64, _vp, _vp, _vp]),
    ("lb_gpu_ivfsq8_search_bitmap_device_ctx", _i, [_vp, _i64, _vp, _i, _i, _vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    ("lb_gpu_ivfsq8_set_filter", _i, [_vp, _vp, _i64]),
    ("lb_gpu_ivfsq8_filter_int64", _i, [_vp, _vp, _i64, _i64, _i, _vp, _i64, _i]),
    ("lb_gpu_ivfsq8_filter_float32", _i, [_vp, _vp, _i64, C.c_float, _i, _vp, _i64, _i]),
    ("lb_gpu_ivfsq8_nvisible", _i64, [_vp]),
    ("lb_gpu_ivfsq8_last_search_stats", _i, [_vp, C.POINTER(C.c_int64)]),
    ("lb_gpu_ivfsq8_set_profiling", _i, [_vp, _i]),
    ("lb_gpu_ivfsq8_last_timing", _i, [_vp, _vp]),
    ("lb_gpu_ivfsq8_last_build_timing", _i, [_vp, _vp]),
    ("lb_gpu_ivfsq8_remove", _i, [_vp, _i64, _vp, C.POINTER(C.c_int64)]),
    ("lb_gpu_ivfsq8_remove_device", _i, [_vp, _i64, _vp, C.POINTER(C.c_int64)]),
    ("lb_gpu_ivfsq8_remove_rows", _i, [_vp, _i64, _vp, C.POINTER(C.c_int64)]),
    ("lb_gpu_ivfsq8_nlive", _i64, [_vp]),
    ("lb_gpu_ivfsq8_ndeleted", _i64, [_vp]),
    ("lb_gpu_ivfsq8_compact", _i, [_vp, _vp, _i64]),
    ("lb_gpu_ivfbq_new", _vp, [_i, _i, _i, _i, _vp, _ip]),
    ("lb_gpu_ivfbq_free", None, [_vp]),
    ("lb_gpu_ivfbq_last_error", C.c_char_p, [_vp]),
    ("lb_gpu_ivfbq_dims", _i, [_vp]),
    ("lb_gpu_ivfbq_words", _i, [_vp]),
    ("lb_gpu_ivfbq_order", _i, [_vp]),
    ("lb_gpu_ivfbq_nlist", _i, [_vp]),
    ("lb_gpu_ivfbq_ntotal", _i64, [_vp]),
    ("lb_gpu_ivfbq_hbm_bytes", _i64, [_vp]),
    ("lb_gpu_ivfbq_get_centroids", _i, [_vp, _vp]),
    ("lb_gpu_ivfbq_reserve", _i, [_vp, _i64]),
    ("lb_gpu_ivfbq_add", _i, [_vp, _i64, _vp, _vp]),
    ("lb_gpu_ivfbq_add_device", _i, [_vp, _i64, _vp, _vp]),
    ("lb_gpu_ivfbq_get_codes", _i, [_vp, _i64, _i64, _vp]),
    ("lb_gpu_ivfbq_list_sizes", _i, [_vp, _vp]),
    ("lb_gpu_ivfbq_assignments", _i, [_vp, _i64, _i64, _vp]),
    ("lb_gpu_ivfbq_search", _i, [_vp, _i64, _vp, _i, _i, _vp, _vp]),
    ("lb_gpu_ivfbq_search_ctx", _i, [_vp, _i64, _vp, _i, _i, _vp, _vp, _vp]),
    ("lb_gpu_ivfbq_search_device_ctx", _i, [_vp, _i64, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    ("lb_gpu_ivfbq_set_filter", _i, [_vp, _vp, _i64]),
    ("lb_gpu_ivfbq_filter_int64", _i, [_vp, _vp, _i64, _i64, _i, _vp, _i64, _i]),
    ("lb_gpu_ivfbq_filter_float32", _i, [_vp, _vp, _i64, C.c_float, _i, _vp, _i64, _i]),
    ("lb_gpu_ivfbq_nvisible", _i64, [_vp]),
    ("lb_gpu_ivfbq_last_search_stats", _i, [_vp, C.POINTER(C.c_int64)]),
    ("lb_gpu_ivfbq_set_profiling", _i, [_vp, _i]),
    ("lb_gpu_ivfbq_last_timing", _i, [_vp, _vp]),
    ("lb_gpu_ivfbq_last_build_timing", _i, [_vp, _vp]),
    ("lb_gpu_merge_topk_device", _i, [_i, _i, _i64, _i, _vp, _vp, _vp, _vp, _vp]),
    ("lb_gpu_merge_topk_packed_device", _i, [_i, _i, _i64, _i, _vp, _vp, _vp, _vp]),
    ("lb_gpu_rrf_fuse_device", _i, [_i, _i64, _i, _vp, _i, _vp, _i, _i, _vp, _vp, _vp]),
    ("lb_gpu_rrf_fuse", _i, [_i, _i64, _i, _vp, _i, _vp, _i, _i, _vp, _vp]),
    ("lb_gpu_fill_uniform_device", _i, [_i, _vp, _i64, _u64, _i64, _vp]),
    ("lb_gpu_fill_codes_device", _i, [_i, _vp, _i64, _u64, _i64, _vp]),
    ("lb_gpu_fill_uniform_rows_device", _i, [_i, _vp, _vp, _i64, _i, _u64, _vp]),
    ("lb_gpu_shader_clock_mhz", C.c_double, [_i, _i]),
    ("lb_flight_datasets_new", _vp, []),
    ("lb_flight_datasets_free", None, [_vp]),
    ("lb_flight_datasets_put", _i, [_vp, C.c_char_p, _vp]),
    ("lb_flight_vector_search_exchange", _i, [_vp, _vp, _sz, C.POINTER(_vp), C.POINTER(_sz), C.c_char_p, _sz]),
    ("lb_flight_encode_results", _i, [_vp, _vp, _i64, C.POINTER(_vp), C.POINTER(_sz)]),
    ("lb_flight_free_buffer", None, [_vp]),
    ("lb_flight_index_add_ipc", _i, [_vp, _vp, _sz, C.POINTER(_i64), C.c_char_p, _sz]),
    ("lb_gpu_comm_init_all", _vp, [_i, _vp, _ip]),
    ("lb_gpu_comm_get_unique_id", _i, [_vp]),
    ("lb_gpu_comm_init_rank", _vp, [_i, _i, _i, _vp, _ip]),
    ("lb_gpu_comm_init_host", _vp, [_i, _i, _i, _vp, _vp, _ip]),
    ("lb_gpu_comm_free", None, [_vp]),
    ("lb_gpu_comm_prepare", _i, [_vp, _i64, _i]),
    ("lb_gpu_comm_nranks", _i, [_vp]),
    ("lb_gpu_comm_rank", _i, [_vp]),
    ("lb_gpu_comm_last_error", C.c_char_p, [_vp]),
    ("lb_gpu_comm_search_device", _i, [_vp, _vp, _i64, _vp, _i, _vp, _vp, _vp]),
    ("lb_gpu_comm_search_all", _i, [_vp, _vp, _i64, _vp, _i, _vp, _vp]),
    ("lb_gpu_index_set_profiling", _i, [_vp, _i]),
    ("lb_gpu_index_last_timing", _i, [_vp, _vp, _vp]),
]


def _bind(path, extra=()):
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: build it with `python -m longbow_amd.build{' --diag' if extra else ''}` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    lib = C.CDLL(path)
    for name, res, args in list(SIGNATURES) + list(extra):
        fn = getattr(lib, name)  # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    return lib


def load():
    """dlopen the HIP library and bind every declared symbol (no GPU needed for this).

    Note for processes that also use PyTorch-ROCm (bench.py, sharded search): import torch BEFORE
    the first call here.  torch ships its own HIP runtime and must initialise first."""
    global _lib
    if _lib is None:
        _lib = _bind(SO_PATH)
    return _lib


# Test hooks exist ONLY in the diagnostic build (liblongbow_gpu_diag.so, -DLB_DIAG):
# tests that force a fallback path create their handles on this library (Index(cfg, lib=load_diag())).
DIAG_SO_PATH = os.path.join(_HERE, "liblongbow_gpu_diag.so")
DIAG_SIGNATURES = [
    ("lb_debug_set_sample_tau", None, [_i]),
    ("lb_debug_vmm_fail_next", None, [_i]),
    ("lb_debug_fused_fail_next", None, [_i]),
    ("lb_debug_tin_withhold_next", None, [_i]),
    ("lb_debug_search_fail_next", None, [_i]),
    ("lb_debug_set_add_register_min", None, [C.c_longlong]),
    ("lb_debug_sample_plan", None, [C.c_longlong, _i, C.c_uint, C.c_uint, C.POINTER(C.c_longlong)]),
    ("lb_debug_cand_geometry", None, [_i, C.POINTER(C.c_int), C.POINTER(C.c_uint)]),
    ("lb_debug_last_wide_rows", _i, []),
    ("lb_debug_set_wide256_min_tiles", None, [_i]),
    ("lb_debug_set_compact_round_rows", None, [C.c_longlong]),
]
_diag = None


def load_diag():
    global _diag
    if _diag is None:
        _diag = _bind(DIAG_SO_PATH, DIAG_SIGNATURES)
    return _diag


def require_gpu(device=0):
    lib = load()
    n = lib.lb_gpu_device_count()
    if n <= 0 or device >= n:
        raise GPUNotAvailable(3, f"{n} HIP device(s) visible, device {device} requested")
    return lib


def check(rc, handle=None, lib=None, prefix=None):
    """prefix: the handle's family ("lb_gpu_pq", ...), whose <prefix>_last_error has the message; none: a flat index's lb_gpu_last_error"""
    if rc == LB_OK:
        return
    msg = ""
    if handle:
        lib = lib or load()
        raw = getattr(lib, prefix + "_last_error" if prefix else "lb_gpu_last_error")(handle)
        msg = raw.decode() if raw else ""
    if rc == 3:
        raise GPUNotAvailable(rc, msg)
    if rc == 8:
        raise Canceled(rc, msg)
    if rc == 9:
        raise DeadlineExceeded(rc, msg)
    raise LongbowGPUError(rc, msg)
