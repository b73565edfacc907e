"""Histogram rows against its alternatives, on the bench's headline input (tests/test_gpu_bench_data.py: bench_input("cfg2")) and on a
constant batch of the same shape (every sample of a column in one bin: the most contention the LDS counters can see).

For each, the median of `--steps` single timings after warm-up:
  (h)  the histogram launch alone, 256 bins of 256 values, H = 0, no mask (device events around sprintz_mi355x_histogram_rows: its memset
       of d_hist included)
  (hm) the same under a seeded Bernoulli mask of a quarter of the rows
  (h1) the same without a mask at H = 1: a histogram a chunk -- every workgroup's chunks lie in several histograms, so every sample is a
       global atomic; recorded, not promised
  (qt) ChunkedCodec.quantiles([0.5, 0.99]): a coarse pass, the refinement passes and the cumulative sums, end to end by the host clock
  (q)  the query_windows launch at W = 64 and (a) the aggregate_rows launch at W = 64 under the same mask: the other reduce-only modes
  (d)  the route through the decoded batch: decompress_into + a per-column torch.bincount of the high bytes, end to end by the host clock
  (ds) decompress_into + a per-column sort + two picks: the quantiles through the decoded batch, end to end by the host clock
(h) and (hm) are checked against (d), (qt) against (ds).  One JSON line per batch; `--out` writes them behind a line that names the
device, the commit and the library file (SPRINTZ_MI355X_LIB selects an A/B build: csrc/decode_ops.h, SPRINTZ_HIST_MERGE).  Exits non-zero
where a result differs.
  python tools/bench_histogram.py [--steps 20] [--commit TEXT] [--out FILE] [--only-launches]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sprintz_amd as sz  # noqa: E402
from sprintz_amd import _lib  # noqa: E402
from rowdata import bench_input


def median_ms(fn, steps, warmup=3, host=False):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(steps):
        torch.cuda.synchronize()
        if host:
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        else:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
    return round(statistics.median(times), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-launches", action="store_true", help="the histogram launches alone (an A/B build's numbers)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    head = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "commit": args.commit, "steps": args.steps,
            "lib": os.path.basename(_lib.LIB_PATH)}
    print(json.dumps(head), flush=True)
    (codec, esz, D, chunk_len, nchunks), x = bench_input("cfg2", dev)
    cd = sz.ChunkedCodec(codec, esz, D, chunk_len, device=dev)
    cid = _lib.CODEC_DELTA if codec == "delta" else _lib.CODEC_XFF
    R = chunk_len // D
    MB = -(-R // 8)
    W = 8 * esz
    top = (1 << W) - 1
    view = torch.int16 if esz == 2 else torch.int8
    nbins, shift = 256, W - 8
    weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(64)
    ok_rows = torch.rand(nchunks * R, generator=gen, device=dev) < 0.25
    mask = (ok_rows.view(-1, 8).to(torch.int32) * weights).sum(dim=1).to(torch.uint8).view(nchunks, MB)
    dec = torch.empty(nchunks * chunk_len, dtype=cd.dtype, device=dev)
    hist = torch.empty((1, D, nbins), dtype=torch.int64, device=dev)
    hist1 = torch.empty((nchunks, D, nbins), dtype=torch.int64, device=dev)
    nwin = R // 64
    mn = torch.empty(nchunks * nwin * D, dtype=cd.dtype, device=dev)
    mx = torch.empty(nchunks * nwin * D, dtype=cd.dtype, device=dev)
    sm = torch.empty(nchunks * nwin * D, dtype=torch.int64, device=dev)
    cnt = torch.empty(nchunks * nwin, dtype=torch.int32, device=dev)
    lines = []
    for name in ("headline", "constant"):
        src = x if name == "headline" else torch.full_like(x.view(view), 0x1234 if esz == 2 else 0x25).view(cd.dtype)
        batch = cd.compress(src)
        del src

        def run_h(m=None, H=0, out=hist):
            _lib.check(_lib.histogram_rows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D,
                                           m.data_ptr() if m is not None else None, None, shift, nbins, H, 0, out.data_ptr(), None, stream()))

        def run_q():
            _lib.check(_lib.query_windows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, 64, 7, 0,
                                          mn.data_ptr(), mx.data_ptr(), sm.data_ptr(), None, stream()))

        def run_a():
            _lib.check(_lib.aggregate_rows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, mask.data_ptr(), 64, 15, 0,
                                           mn.data_ptr(), mx.data_ptr(), sm.data_ptr(), cnt.data_ptr(), None, stream()))

        def run_d(sel=None):
            cd.decompress_into(batch.data, batch.offsets, nchunks, dec)
            v = ((dec.view(view).to(torch.int32) & top) >> shift).view(-1, D)
            if sel is not None:
                v = v[sel]
            return torch.stack([torch.bincount(v[:, d], minlength=nbins) for d in range(D)])

        def run_ds():
            cd.decompress_into(batch.data, batch.offsets, nchunks, dec)
            v = (dec.view(view).to(torch.int32) & top).view(-1, D)
            s = torch.sort(v, dim=0).values
            n = s.shape[0]
            return torch.stack([s[max(math.ceil(q * n), 1) - 1] for q in (0.5, 0.99)])

        def run_qt():
            return cd.quantiles(batch, [0.5, 0.99])

        run_h()
        torch.cuda.synchronize()
        ok_h = torch.equal(hist[0], run_d())
        run_h(mask)
        torch.cuda.synchronize()
        ok_hm = torch.equal(hist[0], run_d(ok_rows))
        run_h(None, 1, hist1)
        torch.cuda.synchronize()
        run_h()
        torch.cuda.synchronize()
        ok_h1 = torch.equal(hist1.sum(dim=0), hist[0])
        rec = {"batch": name, "codec": codec, "elem_bytes": esz, "ndims": D, "chunk_len": chunk_len, "nchunks": nchunks, "nbins": nbins, "shift": shift,
               "ok": bool(ok_h and ok_hm and ok_h1), "rows": nchunks * R, "rows_selected": int(ok_rows.sum().item()),
               "h_histogram_launch_ms": median_ms(run_h, args.steps),
               "hm_histogram_quarter_mask_launch_ms": median_ms(lambda: run_h(mask), args.steps),
               "h1_histogram_per_chunk_launch_ms": median_ms(lambda: run_h(None, 1, hist1), args.steps),
               "compressed_bytes": batch.total_bytes(), "decoded_bytes": nchunks * chunk_len * esz}
        if not args.only_launches:
            got_q = run_qt().view(view).to(torch.int32) & top
            rec["ok"] = bool(rec["ok"] and torch.equal(got_q, run_ds()))
            rec.update({"qt_quantiles_ms": median_ms(run_qt, args.steps, host=True),
                        "q_query_windows_launch_ms": median_ms(run_q, args.steps),
                        "a_aggregate_launch_ms": median_ms(run_a, args.steps),
                        "d_decompress_torch_bincount_ms": median_ms(run_d, args.steps, host=True),
                        "ds_decompress_torch_sort_ms": median_ms(run_ds, args.steps, host=True)})
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del batch
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(head) + "\n")
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
    if not all(r["ok"] for r in lines):
        sys.exit("histogram_rows / quantiles differ from decompress + torch")


if __name__ == "__main__":
    main()
