"""Extrema rows against its alternatives, on the bench's headline input (tests/test_gpu_bench_data.py: bench_input("cfg2")).

A seeded Bernoulli mask of a quarter of the rows (and no mask), 64-row windows.  In one process, the median of `--steps` single timings
after warm-up:
  (e4) the extrema launch with min | max | argmin | argmax (device events around sprintz_mi355x_extrema_rows)
  (e8) the same with all eight ops
  (a)  the aggregate_rows launch of the same batch, mask and window, all four ops -- the comparison point
  (q)  the query_windows launch at the same window: the same decode without a mask -- the floor
  (d)  decompress_into + torch.min / torch.max with indices over the same windows (masked), end to end by the host clock
and on a constant batch of the same shape: (e4), (e8) and (a) under the delta codec, whose runs take the O(windows) shortcut, and under
FIRE, whose runs are replayed row by row -- the shortcut's price tag.
(e8) is checked against (d)'s decoded batch once per mask: min, max, the FIRST selected row holding each, first, last, their rows, the
count.  One JSON line per measurement set; `--out` writes them behind a line that names the device and the commit.  Exits non-zero where
the launch differs from torch.
  python tools/bench_extrema.py [--steps 20] [--commit TEXT] [--out FILE]
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
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    head = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "commit": args.commit, "steps": args.steps}
    print(json.dumps(head), flush=True)
    (codec, esz, D, chunk_len, nchunks), x = bench_input("cfg2", dev)
    R = chunk_len // D
    MB = -(-R // 8)
    W = 64
    assert R % W == 0
    nwin = R // W
    m = nchunks * nwin
    top = (1 << (8 * esz)) - 1
    view = torch.int16 if esz == 2 else torch.int8
    NO = 0xFFFFFFFF
    weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(64)
    ok_quarter = torch.rand(nchunks * R, generator=gen, device=dev) < 0.25
    quarter = (ok_quarter.view(-1, 8).to(torch.int32) * weights).sum(dim=1).to(torch.uint8).view(nchunks, MB)
    out_e = {k: torch.empty(m * D, dtype=torch.uint16 if esz == 2 else torch.uint8, device=dev) for k in ("min", "max", "first", "last")}
    out_w = {k: torch.empty(m * D, dtype=torch.int32, device=dev) for k in ("argmin", "argmax")}
    out_w["rows"] = torch.empty(m * 2, dtype=torch.int32, device=dev)
    out_w["count"] = torch.empty(m, dtype=torch.int32, device=dev)
    sm = torch.empty(m * D, dtype=torch.int64, device=dev)
    lines = []

    def launches(cd, batch, mask):
        cid = _lib.CODEC_DELTA if cd.codec == "delta" else _lib.CODEC_XFF
        mp = mask.data_ptr() if mask is not None else None

        def run_e(ops):
            _lib.check(_lib.extrema_rows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, mp, W, ops, 0,
                                         out_e["min"].data_ptr(), out_e["max"].data_ptr(), out_w["argmin"].data_ptr(), out_w["argmax"].data_ptr(),
                                         out_e["first"].data_ptr(), out_e["last"].data_ptr(), out_w["rows"].data_ptr(), out_w["count"].data_ptr(),
                                         None, stream()))

        def run_a():
            _lib.check(_lib.aggregate_rows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, mp, W, 15, 0,
                                           out_e["min"].data_ptr(), out_e["max"].data_ptr(), sm.data_ptr(), out_w["count"].data_ptr(), None, stream()))

        def run_q():
            _lib.check(_lib.query_windows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, W, 7, 0,
                                          out_e["min"].data_ptr(), out_e["max"].data_ptr(), sm.data_ptr(), None, stream()))
        return run_e, run_a, run_q

    # ---- the headline batch
    cd = sz.ChunkedCodec(codec, esz, D, chunk_len, device=dev)
    batch = cd.compress(x)
    del x
    dec = torch.empty(nchunks * chunk_len, dtype=cd.dtype, device=dev)
    full = torch.full((nchunks, MB), 0xFF, dtype=torch.uint8, device=dev)
    for name, mask, ok_rows in (("p=1/4", quarter, ok_quarter), ("none", None, None)):
        run_e, run_a, run_q = launches(cd, batch, mask)

        def run_d():
            cd.decompress_into(batch.data, batch.offsets, nchunks, dec)
            v = (dec.view(view).to(torch.int32) & top).view(nchunks, nwin, W, D)
            if ok_rows is None:
                return v, None, v.min(dim=2), v.max(dim=2)
            ok = ok_rows.view(nchunks, nwin, W, 1)
            return v, ok, torch.where(ok, v, top + 1).min(dim=2), torch.where(ok, v, -1).max(dim=2)

        run_e(255)
        torch.cuda.synchronize()
        v, ok, (mn, _), (mx, _) = run_d()
        okb = torch.ones((nchunks, nwin, W, 1), dtype=torch.bool, device=dev) if ok is None else ok
        any_ = okb.any(dim=2)                                              # [nchunks, nwin, 1]
        j = torch.arange(W, device=dev).view(1, 1, W, 1)
        base = (torch.arange(nwin, device=dev) * W).view(1, nwin, 1)
        first_of = lambda hit: torch.where(hit, j, W).amin(dim=2)          # noqa: E731  (the first row along a window where `hit`)
        amin = torch.where(any_, first_of(okb & (v == mn.unsqueeze(2))) + base, NO)
        amax = torch.where(any_, first_of(okb & (v == mx.unsqueeze(2))) + base, NO)
        fr = first_of(okb)                                                 # [nchunks, nwin, 1]
        lr = torch.where(okb, j, -1).amax(dim=2)
        pick = lambda r: torch.where(any_, v.gather(2, r.clamp(0, W - 1).unsqueeze(2).expand(-1, -1, 1, D)).squeeze(2), 0)   # noqa: E731
        want = {"min": torch.where(any_, mn, top), "max": torch.where(any_, mx, 0), "argmin": amin, "argmax": amax, "first": pick(fr), "last": pick(lr),
                "rows": torch.where(any_, torch.cat([fr, lr], dim=2) + base, NO), "count": okb.sum(dim=(2, 3))}
        got = {k: t.view(view).to(torch.int64) & top for k, t in out_e.items()}
        got.update({k: t.to(torch.int64) & NO for k, t in out_w.items()})
        bad = [k for k in want if not torch.equal(got[k].view(-1), want[k].to(torch.int64).reshape(-1))]
        del v, ok, okb, mn, mx, want, got
        rec = {"data": "headline", "mask": name, "window_rows": W, "codec": codec, "elem_bytes": esz, "ndims": D, "chunk_len": chunk_len, "nchunks": nchunks,
               "ok": not bad, "differs": bad, "windows": m,
               "e4_extrema_min_max_argmin_argmax_ms": median_ms(lambda: run_e(15), args.steps),
               "e8_extrema_all_eight_ms": median_ms(lambda: run_e(255), args.steps),
               "e2_extrema_min_max_ms": median_ms(lambda: run_e(3), args.steps),
               "a_aggregate_launch_ms": median_ms(run_a, args.steps) if mask is not None else None,
               "a_aggregate_full_mask_ms": median_ms(launches(cd, batch, full)[1], args.steps) if mask is None else None,
               "q_query_windows_launch_ms": median_ms(run_q, args.steps),
               "d_decompress_torch_min_max_indices_ms": median_ms(run_d, args.steps, host=True),
               "compressed_bytes": batch.total_bytes(), "decoded_bytes": nchunks * chunk_len * esz}
        rec["e4_over_aggregate"] = round(rec["e4_extrema_min_max_argmin_argmax_ms"] / (rec["a_aggregate_launch_ms"] or rec["a_aggregate_full_mask_ms"]), 3)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    del dec, batch
    # ---- a constant batch of the same shape: the delta codec's run shortcut against FIRE's row loop
    const = torch.full((nchunks * chunk_len,), 0x1234 if esz == 2 else 0xA5, dtype=torch.int32, device=dev).to(view).view(cd.dtype)
    for cname in ("delta", "xff"):
        cc = sz.ChunkedCodec(cname, esz, D, chunk_len, device=dev)
        cb = cc.compress(const)
        for name, mask in (("p=1/4", quarter), ("none", None)):
            run_e, run_a, run_q = launches(cc, cb, mask)
            run_e(255)
            torch.cuda.synchronize()
            cnt_ok = torch.equal(out_w["count"].view(nchunks, nwin).to(torch.int64),
                                 (ok_quarter.view(nchunks, nwin, W).sum(dim=2) if mask is not None else torch.full((nchunks, nwin), W, device=dev)))
            arg_ok = torch.equal(out_w["argmin"].view(m, D), out_w["rows"].view(m, 2)[:, :1].expand(-1, D))       # constant: the first selected row
            rec = {"data": "constant", "mask": name, "window_rows": W, "codec": cname, "run_shortcut": cname == "delta", "ok": bool(cnt_ok and arg_ok),
                   "e4_extrema_min_max_argmin_argmax_ms": median_ms(lambda: run_e(15), args.steps),
                   "e8_extrema_all_eight_ms": median_ms(lambda: run_e(255), args.steps),
                   "a_aggregate_launch_ms": median_ms(run_a if mask is not None else launches(cc, cb, full)[1], args.steps),
                   "q_query_windows_launch_ms": median_ms(run_q, args.steps), "compressed_bytes": cb.total_bytes()}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(head) + "\n")
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
    if not all(r["ok"] for r in lines):
        sys.exit("extrema_rows differs from decompress + torch")


if __name__ == "__main__":
    main()
