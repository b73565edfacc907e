"""Times the exact Huff0 writer (sprintz_mi355x_huf0_compress_batch_exact: one code table a chunk, libzstd 1.4.8's
bytes) against the shared-table writer (sprintz_mi355x_huf0_compress_batch) and libzstd's HUF_compress on host
threads, on BASELINE config 4's data (u16 x 8, FIRE, 10 KB chunks; tools/synth.py's walk, as bench.py makes it).
Prints one JSON line per batch size: milliseconds (median of --reps) and the ratio (samples bytes / block bytes).

    python tools/huf0_exact_bench.py [--chunks 1250,10000,80000,800000] [--reps 7] [--threads 16]

The phases (X1 = histogram + lengths + tables + sizes, X2 = streams) are read from a kernel trace of the same run."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import sprintz_amd  # noqa: E402
from synth import synth_torch  # noqa: E402


def gpu_ms(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def cpu_ms(streams, threads, reps):
    """HUF_compress of every stream on `threads` host threads (ctypes lets go of the GIL during the call)"""
    try:
        z = C.CDLL("libzstd.so.1")
    except OSError:
        return None, None
    z.HUF_compress.restype = C.c_size_t
    z.HUF_compress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    z.HUF_isError.restype = C.c_uint
    z.HUF_isError.argtypes = [C.c_size_t]
    n = len(streams)
    dst = [np.empty(s.size + 512, np.uint8) for s in streams]
    out = np.zeros(n, np.int64)

    def part(k):
        for c in range(k, n, threads):
            s = streams[c]
            r = z.HUF_compress(dst[c].ctypes.data, dst[c].size, s.ctypes.data, s.size) if s.size else 0
            out[c] = s.size if (r == 0 or z.HUF_isError(r)) else (1 if r == 1 else r)
    ts = []
    with ThreadPoolExecutor(threads) as ex:
        for _ in range(max(1, reps // 3)):
            t0 = time.perf_counter()
            list(ex.map(part, range(threads)))
            ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), int(out.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", default="1250,10000,80000,800000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    for nchunks in [int(v) for v in a.chunks.split(",")]:
        x = synth_torch("walk", 2, nchunks, 5120 // 8, 8, "cuda:0", seed=123, step=8, chunk0=0)
        raw = x.numel() * 2
        cd = sprintz_amd.ChunkedCodec("xff", 2, 8, 5120, device="cuda:0")
        batch = cd.compress(x)
        del x
        torch.cuda.synchronize()
        res = {"chunks": nchunks, "stream_bytes": int(batch.sizes.sum().item())}
        box = {}

        def exact():
            box["e"] = sprintz_amd.huf0_compress_exact(batch)

        def shared():
            box["s"] = sprintz_amd.huf0_compress(batch)
        exact(); shared()
        torch.cuda.synchronize()
        res["exact_ms"] = gpu_ms(exact, a.reps)
        res["shared_ms"] = gpu_ms(shared, a.reps)
        res["exact_ratio"] = raw / int(box["e"][1][-1].item())
        res["shared_ratio"] = raw / int(box["s"][1][-1].item())
        if not a.no_cpu:
            comp, offs, sz = batch.data.cpu().numpy(), batch.offsets.cpu().numpy(), batch.sizes.cpu().numpy()
            streams = [np.ascontiguousarray(comp[int(offs[c]):int(offs[c]) + int(sz[c])]) for c in range(nchunks)]
            ms, tot = cpu_ms(streams, a.threads, a.reps)
            res["libzstd_ms"], res["libzstd_threads"] = ms, a.threads
            if tot is not None:
                res["libzstd_bytes_equal"] = tot == int(box["e"][1][-1].item())
        del box, batch
        torch.cuda.empty_cache()
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
