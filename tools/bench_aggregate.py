"""Aggregate rows against its alternatives, on the bench's headline input (tests/test_gpu_bench_data.py: bench_input("cfg2")).

Four masks -- seeded Bernoulli masks with p = 1, 1/4 and 1/64, and the band predicate of tools/bench_filter.py (columns 0 and D - 1 inside
their own quartiles, mode ALL: a quarter of the rows, in spans) as filter_rows writes it -- at W = 64 and at W = R (one window a chunk).
For each, the median of `--steps` single timings after warm-up:
  (a) the aggregate launch alone, all four ops (device events around sprintz_mi355x_aggregate_rows)
  (q) the query_windows launch at the same W: the same work without a mask -- the floor
  (s) the select_rows launch at the same mask: what it costs to move the selected rows out instead
  (f) the route through the selected rows: [band: filter_rows +] select_rows(ids) + a segmented reduction in torch (scatter_reduce of the
      rows into their windows, int32: torch has no uint16 reductions), end to end by the host clock
  (d) the route through the decoded batch: decompress_into + [band: the torch predicate +] masked reductions over [nchunks, R / W, W, D],
      end to end by the host clock
(a) is checked against (d) once per mask and window.  One JSON line per (mask, W); `--out` writes them behind a line that names the device
and the commit.  Exits non-zero where (a) differs from (d).
  python tools/bench_aggregate.py [--steps 20] [--commit TEXT] [--out FILE]
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
    cd = sz.ChunkedCodec(codec, esz, D, chunk_len, device=dev)
    batch = cd.compress(x)
    del x
    cid = _lib.CODEC_DELTA if codec == "delta" else _lib.CODEC_XFF
    R = chunk_len // D
    MB = -(-R // 8)
    assert R % 64 == 0
    top = (1 << (8 * esz)) - 1
    view = torch.int16 if esz == 2 else torch.int8
    bias = -32768 if esz == 2 else -128
    dec = torch.empty(nchunks * chunk_len, dtype=cd.dtype, device=dev)
    cd.decompress_into(batch.data, batch.offsets, nchunks, dec)
    lo, hi = [0] * D, [top] * D
    for d in sorted({0, D - 1}):
        col = dec.view(-1, D)[:, d].to(torch.int32)
        lo[d] = int(torch.kthvalue(col, int(0.25 * (col.numel() - 1)) + 1).values.item())
        hi[d] = int(torch.kthvalue(col, int(0.75 * (col.numel() - 1)) + 1).values.item())
        del col
    lo_t, hi_t = cd._filter_bounds(lo, hi, "all")
    lo_s, hi_s = lo_t.view(view) ^ bias, hi_t.view(view) ^ bias      # unsigned order = signed order with the sign bit flipped

    def predicate():
        v = dec.view(view).view(-1, D) ^ bias
        return ((v >= lo_s) & (v <= hi_s)).all(dim=1)

    def values32():                                                  # the decoded batch as unsigned values, int32
        return dec.view(view).to(torch.int32) & top

    weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(64)
    lines = []
    for name, p in (("p=1", 1.0), ("p=1/4", 0.25), ("p=1/64", 1.0 / 64), ("band", None)):
        if p is None:
            mask = cd.filter_rows(batch, lo, hi)["mask"]
            get_ok = predicate
        else:
            ok_fixed = torch.rand(nchunks * R, generator=gen, device=dev) < p
            mask = (ok_fixed.view(-1, 8).to(torch.int32) * weights).sum(dim=1).to(torch.uint8).view(nchunks, MB)
            get_ok = lambda ok_fixed=ok_fixed: ok_fixed                  # noqa: E731
        total = int(get_ok().sum().item())
        counts = get_ok().view(nchunks, R).sum(dim=1).to(torch.int32)
        c64 = counts.to(torch.int64)
        bases = (torch.cumsum(c64, 0) - c64).contiguous()
        rows = torch.empty(max(total, 1) * D, dtype=cd.dtype, device=dev)
        for W in (64, R):
            nwin = R // W
            m = nchunks * nwin
            mn = torch.empty(m * D, dtype=cd.dtype, device=dev)
            mx = torch.empty(m * D, dtype=cd.dtype, device=dev)
            sm = torch.empty(m * D, dtype=torch.int64, device=dev)
            cnt = torch.empty(m, dtype=torch.int32, device=dev)

            def run_a():
                _lib.check(_lib.aggregate_rows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, mask.data_ptr(), W, 15, 0,
                                               mn.data_ptr(), mx.data_ptr(), sm.data_ptr(), cnt.data_ptr(), None, stream()))

            def run_q():
                _lib.check(_lib.query_windows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, W, 7, 0,
                                              mn.data_ptr(), mx.data_ptr(), sm.data_ptr(), None, stream()))

            def run_s():
                _lib.check(_lib.select_rows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, mask.data_ptr(),
                                            bases.data_ptr(), total, 0, rows.data_ptr(), None, None, stream()))

            def run_f():
                if p is None:
                    f = cd.filter_rows(batch, lo, hi)
                    got = cd.select_rows(batch, f["mask"], f["counts"], ids=True, check=False)
                else:
                    got = cd.select_rows(batch, mask, counts, ids=True, check=False)
                v = got["rows"].view(view).to(torch.int32) & top
                w = (got["ids"] // W).view(-1, 1).expand(-1, D)
                o_mn = torch.full((m, D), top, dtype=torch.int32, device=dev).scatter_reduce_(0, w, v, "amin")
                o_mx = torch.zeros((m, D), dtype=torch.int32, device=dev).scatter_reduce_(0, w, v, "amax")
                o_sm = torch.zeros((m, D), dtype=torch.int64, device=dev).scatter_add_(0, w, v.to(torch.int64))
                o_cnt = torch.bincount(got["ids"] // W, minlength=m)
                return o_mn, o_mx, o_sm, o_cnt

            def run_d():
                cd.decompress_into(batch.data, batch.offsets, nchunks, dec)
                ok = get_ok().view(nchunks, nwin, W, 1)
                v = values32().view(nchunks, nwin, W, D)
                o_mn = torch.where(ok, v, top).amin(dim=2)
                o_mx = torch.where(ok, v, 0).amax(dim=2)
                o_sm = torch.where(ok, v, 0).sum(dim=2)
                o_cnt = ok.sum(dim=(2, 3))
                return o_mn, o_mx, o_sm, o_cnt

            run_a()
            torch.cuda.synchronize()
            got = (mn.view(view).to(torch.int32) & top, mx.view(view).to(torch.int32) & top, sm.clone(), cnt.to(torch.int64))
            want = run_d()
            ok_d = all(torch.equal(g.view(-1), w.view(-1).to(g.dtype)) for g, w in zip(got, want))
            alt = run_f()
            ok_f = all(torch.equal(g.view(-1), w.view(-1).to(g.dtype)) for g, w in zip(got, alt))
            del want, alt
            rec = {"mask": name, "window_rows": W, "codec": codec, "elem_bytes": esz, "ndims": D, "chunk_len": chunk_len, "nchunks": nchunks,
                   "ok": bool(ok_d and ok_f), "rows": nchunks * R, "rows_selected": total, "windows": m,
                   "a_aggregate_launch_ms": median_ms(run_a, args.steps),
                   "q_query_windows_launch_ms": median_ms(run_q, args.steps),
                   "s_select_launch_ms": median_ms(run_s, args.steps),
                   "f_select_torch_segmented_ms": median_ms(run_f, args.steps, host=True),
                   "d_decompress_torch_masked_ms": median_ms(run_d, args.steps, host=True),
                   "compressed_bytes": batch.total_bytes(), "decoded_bytes": nchunks * chunk_len * esz, "selected_bytes": total * D * esz}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        del rows
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(head) + "\n")
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
    if not all(r["ok"] for r in lines):
        sys.exit("aggregate_rows differs from decompress + torch or from select_rows + torch")


if __name__ == "__main__":
    main()
