"""Group-by rows against its alternatives, on the bench's headline input (tests/test_gpu_bench_data.py: bench_input("cfg2")) and on a
constant batch of the same shape (every row in one bin: the most contention the LDS table can see).  256 key bins of 256 values
(shift 8), key column 0.

For each, the median of `--steps` single timings after warm-up:
  (g)  the group-by launch alone, count and sums, H = 0, no mask (device events around sprintz_mi355x_groupby_rows: its memsets of
       d_count and d_sum included)
  (gm) the same under a seeded Bernoulli mask of a quarter of the rows
  (g1) the same without a mask at H = 1: a table a chunk -- every workgroup's chunks lie in several tables, so every add is a global
       atomic; recorded, not promised
  (gc) COUNT alone and (gs) SUM alone, H = 0, no mask
  (h)  the histogram_rows launch (256 bins, every column), (a) the aggregate_rows launch at W = 64 under the same mask and (q) the
       query_windows launch at W = 64: the other reduce-only modes
  (d)  the route through the decoded batch: decompress_into + torch.bincount of the key bins + index_add_ of the rows, end to end by
       the host clock
(g) and (gm) are checked against (d), (g1) summed over the chunks, (gc) and (gs) against (g), and the count table against (h)'s key
column.  (g1) and (d) are the median of at most 5.  One JSON line per batch; `--out` writes them behind a line that names the device,
the commit and the library file (SPRINTZ_MI355X_LIB selects an A/B build: csrc/decode_ops.h, SPRINTZ_GBY_MERGE).  Exits non-zero where
a result differs.
  python tools/bench_groupby.py [--steps 20] [--commit TEXT] [--out FILE] [--only-launches]
"""
import argparse
import ctypes as C
import json
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
    ap.add_argument("--only-launches", action="store_true", help="the group-by launches alone (an A/B build's numbers)")
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
    key, nbins, shift = 0, 256, W - 8
    weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(64)
    ok_rows = torch.rand(nchunks * R, generator=gen, device=dev) < 0.25
    mask = (ok_rows.view(-1, 8).to(torch.int32) * weights).sum(dim=1).to(torch.uint8).view(nchunks, MB)
    dec = torch.empty(nchunks * chunk_len, dtype=cd.dtype, device=dev)
    cnt = torch.empty((1, nbins), dtype=torch.int64, device=dev)
    tot = torch.empty((1, nbins, D), dtype=torch.int64, device=dev)
    cnt_b = torch.empty_like(cnt)
    tot_b = torch.empty_like(tot)
    cnt1 = torch.empty((nchunks, nbins), dtype=torch.int64, device=dev)
    tot1 = torch.empty((nchunks, nbins, D), dtype=torch.int64, device=dev)
    hist = torch.empty((1, D, nbins), dtype=torch.int64, device=dev)
    nwin = R // 64
    mn = torch.empty(nchunks * nwin * D, dtype=cd.dtype, device=dev)
    mx = torch.empty(nchunks * nwin * D, dtype=cd.dtype, device=dev)
    sm = torch.empty(nchunks * nwin * D, dtype=torch.int64, device=dev)
    acnt = torch.empty(nchunks * nwin, dtype=torch.int32, device=dev)
    lines = []
    for name in ("headline", "constant"):
        src = x if name == "headline" else torch.full_like(x.view(view), 0x1234 if esz == 2 else 0x25).view(cd.dtype)
        batch = cd.compress(src)
        del src

        def run_g(m=None, H=0, ops=3, c=cnt, t=tot):
            _lib.check(_lib.groupby_rows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D,
                                         m.data_ptr() if m is not None else None, key, 0, shift, nbins, H, ops, 0,
                                         c.data_ptr() if ops & 1 else None, t.data_ptr() if ops & 2 else None, None, stream()))

        def run_h():
            _lib.check(_lib.histogram_rows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, None, None, shift, nbins, 0, 0,
                                           hist.data_ptr(), None, stream()))

        def run_q():
            _lib.check(_lib.query_windows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, 64, 7, 0,
                                          mn.data_ptr(), mx.data_ptr(), sm.data_ptr(), None, stream()))

        def run_a():
            _lib.check(_lib.aggregate_rows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, mask.data_ptr(), 64, 15, 0,
                                           mn.data_ptr(), mx.data_ptr(), sm.data_ptr(), acnt.data_ptr(), None, stream()))

        def run_d(sel=None):
            cd.decompress_into(batch.data, batch.offsets, nchunks, dec)
            v = (dec.view(view).to(torch.int64) & top).view(-1, D)
            if sel is not None:
                v = v[sel]
            b = v[:, key] >> shift
            return torch.bincount(b, minlength=nbins), torch.zeros((nbins, D), dtype=torch.int64, device=dev).index_add_(0, b, v)

        run_g()
        torch.cuda.synchronize()
        dc, ds = run_d()
        ok_g = torch.equal(cnt[0], dc) and torch.equal(tot[0], ds)
        run_g(mask)
        torch.cuda.synchronize()
        dc, ds = run_d(ok_rows)
        ok_gm = torch.equal(cnt[0], dc) and torch.equal(tot[0], ds)
        del dc, ds
        run_g()
        run_g(None, 1, 3, cnt1, tot1)
        torch.cuda.synchronize()
        ok_g1 = torch.equal(cnt1.sum(dim=0), cnt[0]) and torch.equal(tot1.sum(dim=0), tot[0])
        run_g(None, 0, 1, cnt_b, tot_b)
        run_g(None, 0, 2, cnt_b, tot_b)
        torch.cuda.synchronize()
        ok_ops = torch.equal(cnt_b, cnt) and torch.equal(tot_b, tot)
        run_h()
        torch.cuda.synchronize()
        ok_h = torch.equal(hist[0, key], cnt[0])            # the count table is the key column's histogram
        rec = {"batch": name, "codec": codec, "elem_bytes": esz, "ndims": D, "chunk_len": chunk_len, "nchunks": nchunks, "key": key, "nbins": nbins,
               "shift": shift, "ok": bool(ok_g and ok_gm and ok_g1 and ok_ops and ok_h), "rows": nchunks * R, "rows_selected": int(ok_rows.sum().item()),
               "g_groupby_launch_ms": median_ms(run_g, args.steps),
               "gm_groupby_quarter_mask_launch_ms": median_ms(lambda: run_g(mask), args.steps),
               "g1_groupby_per_chunk_launch_ms": median_ms(lambda: run_g(None, 1, 3, cnt1, tot1), min(args.steps, 5)),
               "gc_groupby_count_only_launch_ms": median_ms(lambda: run_g(None, 0, 1), args.steps),
               "gs_groupby_sum_only_launch_ms": median_ms(lambda: run_g(None, 0, 2), args.steps),
               "compressed_bytes": batch.total_bytes(), "decoded_bytes": nchunks * chunk_len * esz}
        if not args.only_launches:
            rec.update({"h_histogram_launch_ms": median_ms(run_h, args.steps),
                        "a_aggregate_launch_ms": median_ms(run_a, args.steps),
                        "q_query_windows_launch_ms": median_ms(run_q, args.steps),
                        "d_decompress_torch_bincount_index_add_ms": median_ms(run_d, min(args.steps, 5), warmup=1, host=True)})
            rec["g_over_h"] = round(rec["g_groupby_launch_ms"] / rec["h_histogram_launch_ms"], 3)
            rec["d_over_g"] = round(rec["d_decompress_torch_bincount_index_add_ms"] / rec["g_groupby_launch_ms"], 1)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del batch
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(head) + "\n")
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
    if not all(r["ok"] for r in lines):
        sys.exit("groupby_rows differs from decompress + torch")


if __name__ == "__main__":
    main()
