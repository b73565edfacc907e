"""Moments rows against its alternatives, on the bench's headline input (tests/test_gpu_bench_data.py: bench_input("cfg2")) and on a
constant batch of the same shape (one delta run a chunk: the run shortcut, where the decode itself is nearly free).

For each, the median of `--steps` single timings after warm-up, W = 64:
  (m3)  the moments launch alone, count | sum | sumsq, under a seeded Bernoulli mask of a quarter of the rows (device events around
        sprintz_mi355x_moments_rows)
  (m4)  the same with all four ops, the reference column 3: the cross products and the exchange of the reference column's rows
  (m3n) (m4n) both without a mask: every row
  (a)   the aggregate_rows launch, all four ops, under the same mask; (q) the query_windows launch: the other reduce-only modes
  (d)   the route through the decoded batch: decompress_into + the same four sums in torch on int64, end to end by the host clock
(m4) and (m4n) are checked against (d) entry for entry, (m3) / (m3n) against (m4) / (m4n).  One JSON line per batch; `--out` writes them
behind a line that names the device, the commit and the library file (SPRINTZ_MI355X_LIB selects an A/B build).  Exits non-zero where a
result differs.
  python tools/bench_moments.py [--steps 20] [--commit TEXT] [--out FILE] [--only-launches] [--nchunks N]
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
    ap.add_argument("--only-launches", action="store_true", help="the moments launches alone (an A/B build's numbers)")
    ap.add_argument("--nchunks", type=int, default=0, help="the first N chunks of the input alone (0: all of it)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    head = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "commit": args.commit, "steps": args.steps,
            "lib": os.path.basename(_lib.LIB_PATH)}
    print(json.dumps(head), flush=True)
    (codec, esz, D, chunk_len, nchunks), x = bench_input("cfg2", dev)
    if args.nchunks:
        nchunks = min(nchunks, args.nchunks)
        x = x[:nchunks * chunk_len].clone()
    cd = sz.ChunkedCodec(codec, esz, D, chunk_len, device=dev)
    cid = _lib.CODEC_DELTA if codec == "delta" else _lib.CODEC_XFF
    R = chunk_len // D
    MB = -(-R // 8)
    top = (1 << (8 * esz)) - 1
    view = torch.int16 if esz == 2 else torch.int8
    Wn, ref = 64, 3
    nwin = R // Wn
    weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(64)
    ok_rows = torch.rand(nchunks * R, generator=gen, device=dev) < 0.25
    mask = (ok_rows.view(-1, 8).to(torch.int32) * weights).sum(dim=1).to(torch.uint8).view(nchunks, MB)
    dec = torch.empty(nchunks * chunk_len, dtype=cd.dtype, device=dev)
    mn = torch.empty(nchunks * nwin * D, dtype=cd.dtype, device=dev)
    mx = torch.empty(nchunks * nwin * D, dtype=cd.dtype, device=dev)
    out = {k: torch.empty(nchunks * nwin * D, dtype=torch.int64, device=dev) for k in ("sum", "sumsq", "cross", "sum3", "sumsq3", "agg")}
    cnt = torch.empty(nchunks * nwin, dtype=torch.int32, device=dev)
    lines = []
    for name in ("headline", "constant"):
        src = x if name == "headline" else torch.full_like(x.view(view), 0x1234 if esz == 2 else 0x25).view(cd.dtype)
        batch = cd.compress(src)
        del src

        def run_m(ops, m=None, three=False):
            s, q = (out["sum3"], out["sumsq3"]) if three else (out["sum"], out["sumsq"])
            _lib.check(_lib.moments_rows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D,
                                         m.data_ptr() if m is not None else None, Wn, ops, ref, 0, cnt.data_ptr(), s.data_ptr(), q.data_ptr(),
                                         out["cross"].data_ptr() if ops & 8 else None, None, stream()))

        def run_q():
            _lib.check(_lib.query_windows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, Wn, 7, 0,
                                          mn.data_ptr(), mx.data_ptr(), out["agg"].data_ptr(), None, stream()))

        def run_a():
            _lib.check(_lib.aggregate_rows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, mask.data_ptr(), Wn, 15, 0,
                                           mn.data_ptr(), mx.data_ptr(), out["agg"].data_ptr(), cnt.data_ptr(), None, stream()))

        def run_d(sel=None):
            cd.decompress_into(batch.data, batch.offsets, nchunks, dec)
            v = (dec.view(view).to(torch.int64) & top).view(-1, D)
            if sel is not None:
                v = v * sel.view(-1, 1)
            n = (sel.view(-1, Wn).sum(dim=1) if sel is not None else torch.full((nchunks * nwin,), Wn, device=dev)).to(torch.int32)
            return n, v.view(-1, Wn, D).sum(dim=1).view(-1), (v * v).view(-1, Wn, D).sum(dim=1).view(-1), \
                (v * v[:, ref:ref + 1]).view(-1, Wn, D).sum(dim=1).view(-1)

        ok = True
        for m, sel in ((mask, ok_rows), (None, None)):
            run_m(15, m)
            run_m(7, m, three=True)
            torch.cuda.synchronize()
            n, s, q, p = run_d(sel)
            ok = ok and torch.equal(cnt, n) and torch.equal(out["sum"], s) and torch.equal(out["sumsq"], q) and torch.equal(out["cross"], p)
            ok = ok and torch.equal(out["sum3"], s) and torch.equal(out["sumsq3"], q)
            del n, s, q, p
        rec = {"batch": name, "codec": codec, "elem_bytes": esz, "ndims": D, "chunk_len": chunk_len, "nchunks": nchunks, "window_rows": Wn, "ref": ref,
               "ok": bool(ok), "rows": nchunks * R, "rows_selected": int(ok_rows.sum().item()),
               "m3_moments_quarter_mask_launch_ms": median_ms(lambda: run_m(7, mask, True), args.steps),
               "m4_moments_cross_quarter_mask_launch_ms": median_ms(lambda: run_m(15, mask), args.steps),
               "m3n_moments_no_mask_launch_ms": median_ms(lambda: run_m(7, None, True), args.steps),
               "m4n_moments_cross_no_mask_launch_ms": median_ms(lambda: run_m(15, None), args.steps),
               "a_aggregate_launch_ms": median_ms(run_a, args.steps),
               "compressed_bytes": batch.total_bytes(), "decoded_bytes": nchunks * chunk_len * esz}
        rec["m4_over_aggregate"] = round(rec["m4_moments_cross_quarter_mask_launch_ms"] / rec["a_aggregate_launch_ms"], 3)
        if not args.only_launches:
            rec.update({"q_query_windows_launch_ms": median_ms(run_q, args.steps),
                        "d_decompress_torch_sums_ms": median_ms(lambda: run_d(ok_rows), args.steps, host=True)})
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del batch
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(head) + "\n")
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
    if not all(r["ok"] for r in lines):
        sys.exit("moments_rows differs from decompress + torch")


if __name__ == "__main__":
    main()
