"""Build liblongbow_gpu.so for gfx950 with hipcc (in-tree, no torch involved).

    python -m longbow_amd.build [--force]

hipcc cross-compiles without a GPU; the .so travels to the GPU box with the tree.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "liblongbow_gpu.so")
OUT_DIAG = os.path.join(HERE, "liblongbow_gpu_diag.so")
SOURCES = ["index.hip", "index_remove.hip", "index_search.hip", "simd_api.hip", "refine.hip", "pq.hip", "pq_train.hip", "bq.hip", "sq8.hip", "ivf.hip", "ivf_train.hip", "ivfpq.hip", "ivfsq8.hip", "ivfbq.hip", "comm.hip", "flight.hip", "kernels_gemm.hip", "kernels_gemm_narrow.hip", "kernels_gemm_tall2.hip", "kernels_gemm_tall16.hip", "kernels_scan.hip", "kernels_select.hip", "kernels_finish.hip",
           "kernels_pq.hip", "kernels_pq2.hip", "kernels_pq_list.hip", "kernels_pq_train.hip", "kernels_filter.hip", "kernels_i8.hip", "kernels_bq.hip", "kernels_sq8.hip", "kernels_countsel.hip", "kernels_index_call.hip", "kernels_ivf.hip", "kernels_ivf_call.hip", "kernels_ivf_f16.hip", "kernels_ivf_i8.hip", "kernels_ivf_train.hip", "kernels_ivfpq.hip", "kernels_ivfsq8.hip", "kernels_ivfbq.hip", "kernels_refine.hip", "kernels_remove.hip"]
HEADERS = ["lb_device.h", "lb_exact.h", "lb_admit.h", "lb_host.h", "lb_handle.h", "lb_index.h", "lb_combine.h", "lb_select.h", "lb_countsel.h", "lb_ivf.h", "lb_ivf_f16.h", "lb_ivf_i8.h", "lb_i8_exact.h", "lb_ivf_host.h", "lb_list_scan.h", "lb_ivfpq.h", "lb_ivfsq8.h", "lb_ivfbq.h", "lb_refine.h", "lb_remove.h", os.path.join("..", "..", "include", "longbow_gpu.h")]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False, diag=False):
    """diag=True builds liblongbow_gpu_diag.so with -DLB_DIAG: the LB_* numeric tunables read from the environment,
    the lb_debug_* test hooks and the observing counters (tests/ and tools/; select it with LB_GPU_SO=<path>)."""
    srcs = [s for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]
    hdrs = [os.path.join(CSRC, h) for h in HEADERS]
    objs = []
    jobs = []
    out = OUT_DIAG if diag else OUT
    for s in srcs:
        src = os.path.join(CSRC, s)
        obj = os.path.join(CSRC, s.replace(".hip", ".diag.o" if diag else ".o"))
        objs.append(obj)
        if force or _stale(obj, [src] + hdrs):
            jobs.append([HIPCC] + FLAGS + (["-DLB_DIAG"] if diag else []) + ["-c", src, "-o", obj])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + r.stdout + r.stderr)
        return r

    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(run, jobs))
    if force or jobs or _stale(out, objs):
        run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs + ["-ldl", "-lpthread"])
    return out


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True, diag="--diag" in sys.argv))
