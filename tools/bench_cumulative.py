"""Cumulative rows against its alternatives, on the bench's headline input (tests/rowdata.py: bench_input("cfg2"): uint16 x 8, FIRE, 10 KB
chunks, 131 072 chunks) and on BASELINE config 3 at 10 KB (bench_input("cfg3_10k"): uint8 x 80, delta).

Every leg is timed with device events around the work, after 3 warm-ups of each leg, and the legs are INTERLEAVED: a step runs every leg
once, in turn, so that a change of the box's load meets all of them alike; the figure is the median of `--steps` steps.  The legs:
  a        decompress_into alone: the plain decode's launch
  float32  the float_rows float32 launch, and roll8: rolling_rows' sum at W = 8 -- both write the bytes the int32 sum writes on uint16
           (the headline batch only)
  b_*      (a) plus the torch expression for the same result on the decoded tensor, taken as ONE sequence of rows.  torch scans an OUTER
           dimension of a [rows, 8] tensor with a thread a column (profiles/rolling_rows.txt), so every expression scans along the contiguous
           dimension of the transposed tensor and transposes back:
             v = (dec.view(int16 / int8).to(torch.int32) & top).view(-1, D)
             min: v.t().contiguous().cummin(1).values.t().contiguous()       max: ... cummax(1) ...
             sum: v.t().to(torch.int64).contiguous().cumsum(1).t().contiguous()
           Each is first timed on 1 / 64 of the rows; one whose full run would take more than --torch-limit seconds is not run in full: its
           line says so and carries the extrapolation instead.
  c_*      sprintz_mi355x_cumulative_rows on preallocated outputs and scratch -- the totals, the scan and the decode: min alone, max alone,
           the sum alone as int32 and as int64, and all three with either sum
  t_*      the totals pass alone (sprintz_mi355x_query_windows with one window a chunk: the launch cumulative_rows makes first)
c is checked against b once per leg, exactly, where b ran.  The int64 sum's floor is its stores and two reads of the compressed batch at
the HBM rate a copy reaches (6.29 TB/s); the line carries the floor and the fraction of it reached.
--kernels runs the three-op int64 call alone, a few times, for a kernel trace taken around this script (the three launches' own times).
One JSON line per measurement; `--out` writes them behind a line that names the device and the commit.  Exits non-zero where c differs
from b, or where on the headline batch c is not faster than b.
  python tools/bench_cumulative.py [--steps 20] [--commit TEXT] [--out FILE] [--torch-limit 5] [--kernels]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sprintz_amd as sz  # noqa: E402
from sprintz_amd import _lib, rowops  # noqa: E402
from rowdata import bench_input  # noqa: E402

HBM_COPY_TB_S = 6.29
LEGS = (("min", 1, 4), ("max", 2, 4), ("sum32", 4, 4), ("sum64", 4, 8), ("all32", 7, 4), ("all64", 7, 8))


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def interleaved(legs, steps, warmup=3):
    """legs: {name: fn} -> {name: (median ms, min, max)}: every step runs every leg once, in turn"""
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    times = {k: [] for k in legs}
    for _ in range(steps):
        for k, fn in legs.items():
            times[k].append(timed(fn))
    return {k: (round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)) for k, v in times.items()}


def torch_cumulative(v, ops):
    """v: int32 [G, D], the decoded batch as one sequence -> {op: [G, D]}"""
    out = {}
    if ops & 1:
        out["min"] = v.t().contiguous().cummin(1).values.t().contiguous()
    if ops & 2:
        out["max"] = v.t().contiguous().cummax(1).values.t().contiguous()
    if ops & 4:
        out["sum"] = v.t().to(torch.int64).contiguous().cumsum(1).t().contiguous()
    return out


def bench_config(name, dev, steps, stream, headline, torch_limit, kernels_only):
    (codec, esz, D, chunk_len, nchunks), x = bench_input(name, dev)
    cd = sz.ChunkedCodec(codec, esz, D, chunk_len, device=dev)
    batch = cd.compress(x)
    del x
    cid = _lib.CODEC_DELTA if codec == "delta" else _lib.CODEC_XFF
    ne = nchunks * chunk_len
    R = chunk_len // D
    top = (1 << (8 * esz)) - 1
    view_in = torch.int16 if esz == 2 else torch.int8
    comp_bytes = int(batch.offsets[nchunks].item())
    dec = torch.empty(ne, dtype=cd.dtype, device=dev)
    omin, omax = torch.empty(ne, dtype=cd.dtype, device=dev), torch.empty(ne, dtype=cd.dtype, device=dev)
    osum = torch.empty(ne, dtype=torch.int64, device=dev)
    tmp = torch.empty(rowops.cumulative_tmp_bytes(nchunks, D), dtype=torch.uint8, device=dev)
    cout = torch.empty(3 * D, dtype=torch.int64, device=dev)
    tw = [torch.empty(nchunks * D, dtype=cd.dtype, device=dev), torch.empty(nchunks * D, dtype=cd.dtype, device=dev), torch.empty(nchunks * D, dtype=torch.int64, device=dev)]
    shape = {"config": name, "codec": codec, "elem_bytes": esz, "ndims": D, "chunk_len": chunk_len, "nchunks": nchunks, "comp_bytes": comp_bytes}

    def run_a():
        cd.decompress_into(batch.data, batch.offsets, nchunks, dec)

    def decoded(rows=None):
        run_a()
        v = (dec.view(view_in).to(torch.int32) & top).view(-1, D)
        return v if rows is None else v[:rows]

    def run_c(ops, sb):
        _lib.check(_lib.cumulative_rows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, ops, sb, 0,
                                        omin.data_ptr() if ops & 1 else None, omax.data_ptr() if ops & 2 else None, osum.data_ptr() if ops & 4 else None,
                                        None, cout.data_ptr(), tmp.data_ptr(), None, stream()))

    def run_t(ops):
        _lib.check(_lib.query_windows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, (R + 7) // 8 * 8, ops, 0,
                                      tw[0].data_ptr() if ops & 1 else None, tw[1].data_ptr() if ops & 2 else None, tw[2].data_ptr() if ops & 4 else None,
                                      None, stream()))

    if kernels_only:
        for _ in range(5):
            run_c(7, 8)
        torch.cuda.synchronize()
        return [], False

    # ---- the torch route: a rehearsal on 1 / 64 of the rows decides whether the full expression is run
    small = max(R, ne // D // 64)
    full, predicted = {}, {}
    for k, ops in (("min", 1), ("max", 2), ("sum", 4)):
        v = decoded(small)
        torch_cumulative(v, ops)
        t = timed(lambda: torch_cumulative(v, ops))
        predicted[k] = round(t * (ne // D) / small, 1)
        full[k] = predicted[k] < torch_limit * 1000.0
        del v
    torch.cuda.empty_cache()

    lines, bad = [], False
    # ---- exactness: c against b, once per leg
    oks = {}
    for leg, ops, sb in LEGS:
        before = _lib.dispatch_counts()
        run_c(ops, sb)
        after = _lib.dispatch_counts()
        family = {k: after[k] - before[k] for k in after if after[k] != before[k]}
        torch.cuda.synchronize()
        ok = None
        if all(full[k] for k, bit in (("min", 1), ("max", 2), ("sum", 4)) if ops & bit):
            want = torch_cumulative(decoded(), ops)
            ok = True
            if ops & 1:
                ok = ok and torch.equal(omin.view(view_in).to(torch.int32) & top, want["min"].reshape(-1))
            if ops & 2:
                ok = ok and torch.equal(omax.view(view_in).to(torch.int32) & top, want["max"].reshape(-1))
            if ops & 4:
                got = osum if sb == 8 else osum.view(torch.int32)[:ne]
                ok = ok and torch.equal(got, want["sum"].reshape(-1) if sb == 8 else want["sum"].reshape(-1).to(torch.int32))
            del want
            torch.cuda.empty_cache()
        oks[leg] = (ok, family)

    # ---- the timings, interleaved
    legs = {"a": run_a}
    if headline:
        fout = torch.empty(ne, dtype=torch.float32, device=dev)
        rtmp = torch.empty(rowops.rolling_tmp_bytes(nchunks, 8, D, esz), dtype=torch.uint8, device=dev)
        legs["float32"] = lambda: _lib.check(_lib.float_rows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, _lib.FLOAT_F32, None,
                                                            None, 0, fout.data_ptr(), None, stream()))
        legs["roll8"] = lambda: _lib.check(_lib.rolling_rows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, 8, 4, 0, None, None,
                                                            fout.data_ptr(), rtmp.data_ptr(), None, stream()))
    for leg, ops, sb in LEGS:
        legs["c_" + leg] = lambda ops=ops, sb=sb: run_c(ops, sb)
    for k, ops in (("min", 1), ("max", 2), ("sum", 4), ("all", 7)):
        legs["t_" + k] = lambda ops=ops: run_t(ops)
    got = interleaved(legs, steps)
    # (the torch legs run in a block of their own: their int64 temporaries would evict everything the other legs keep in the caches)
    tlegs = {"b_" + k: (lambda ops=ops: torch_cumulative(decoded(), ops)) for k, ops in (("min", 1), ("max", 2), ("sum", 4)) if full[k]}
    got.update(interleaved(tlegs, max(3, steps // 4), warmup=1) if tlegs else {})
    torch.cuda.empty_cache()

    a = got["a"][0]
    lines.append(dict(shape, what="a_decompress", ms=a, lo=got["a"][1], hi=got["a"][2], out_bytes=ne * esz))
    for k in ("float32", "roll8"):
        if k in got:
            lines.append(dict(shape, what=k, ms=got[k][0], lo=got[k][1], hi=got[k][2], out_bytes=ne * 4))
    for k in ("min", "max", "sum"):
        lines.append(dict(shape, what="b_decompress_torch", op=k, ran_in_full=full[k], ms=got["b_" + k][0] if full[k] else None,
                          extrapolated_from_a_64th_ms=predicted[k]))
    for k in ("min", "max", "sum", "all"):
        lines.append(dict(shape, what="totals_pass", ops=k, ms=got["t_" + k][0], lo=got["t_" + k][1], hi=got["t_" + k][2]))
    for leg, ops, sb in LEGS:
        c = got["c_" + leg]
        ok, family = oks[leg]
        parts = [k for k, bit in (("min", 1), ("max", 2), ("sum", 4)) if ops & bit]
        b = sum(got["b_" + k][0] if full[k] else predicted[k] for k in parts) - (len(parts) - 1) * a          # one decompress, every expression
        out_bytes = ne * (esz * bin(ops & 3).count("1") + (sb if ops & 4 else 0))
        floor = (out_bytes + 2 * comp_bytes) / (HBM_COPY_TB_S * 1e9)
        rec = dict(shape, what="cumulative", leg=leg, ops=ops, sum_bytes=sb if ops & 4 else None, launches=family, ok=ok, a_decompress_ms=a, b_decompress_torch_ms=round(b, 4),
                   b_measured=all(full[k] for k in parts), c_cumulative_ms=c[0], c_lo=c[1], c_hi=c[2], totals_ms=got["t_" + ("all" if ops == 7 else parts[0])][0],
                   c_out_bytes=out_bytes, c_over_a=round(c[0] / a, 3), c_over_b=round(c[0] / b, 4), c_out_gb_s=round(out_bytes / c[0] / 1e6, 1),
                   floor_ms=round(floor, 4), floor_fraction=round(floor / c[0], 3))
        lines.append(rec)
        bad = bad or ok is False or (headline and not c[0] < b)
    for rec in lines:
        print(json.dumps(rec), flush=True)
    return lines, bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    ap.add_argument("--torch-limit", type=float, default=5.0, help="seconds: a torch expression whose full run is predicted to take longer is not run in full")
    ap.add_argument("--kernels", action="store_true", help="the three-op int64 call on the headline batch alone, five times: for a kernel trace around this script")
    ap.add_argument("--configs", default="cfg2,cfg3_10k")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    head = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "commit": args.commit, "steps": args.steps}
    print(json.dumps(head), flush=True)
    lines, bad = [], False
    for name in args.configs.split(","):
        got, b = bench_config(name, dev, args.steps, stream, name == "cfg2", args.torch_limit, args.kernels)
        lines += got
        bad = bad or b
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(head) + "\n")
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
