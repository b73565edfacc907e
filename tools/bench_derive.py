"""Derive rows against its alternatives, on the bench's headline input (tests/rowdata.py: bench_input("cfg2"): uint16 x 8, FIRE, 10 KB chunks,
131 072 chunks) and on BASELINE config 3 at 10 KB (bench_input("cfg3_10k"): uint8 x 80, delta -- a shape the generic kernel serves).

Everything in one job, every variant of a shape timed in turn, round after round (`--steps` rounds behind 3 warm-up rounds), device events around
the work; a line gives the median, the fastest and the slowest round:
  decompress                   the plain decode's launch (decompress_into) -- twice a round, first and last, as the job's own spread
  filter_linear                the linear filter's launch with the form a - b: the same arithmetic with one bit out
  project_float32_K1 / _K2     project rows to float32 at the same K: the same output bytes
  derive_*                     the derivation's call on preallocated outputs: a - b as int32 and as float32 (K = 1), a - b and c + d as float32
                               (K = 2), every column's diff as int32 (K = 8: a lag term, scratch and the seam pass)
  torch_*                      the routes they replace: the full decode, then the torch expression on the decoded tensor -- slices, the
                               conversion, the arithmetic, and torch.diff(..., prepend=) for the diff
Each derivation is checked against its torch route once, exactly, and its line says whether its median lies below its torch route's fastest
round (`beats_torch`).  One JSON line per measurement; `--out` writes them behind a line that names the device and the commit.  Exits non-zero
where a result differs.
  python tools/bench_derive.py [--steps 20] [--commit TEXT] [--out FILE]
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


def time_rounds(variants, steps, warmup=3):
    """variants: [(name, fn)] -> {name: [ms, ...]}: every variant once a round, in order, so that a drift of the box meets all of them alike"""
    times = {name: [] for name, _ in variants}
    for r in range(warmup + steps):
        for name, fn in variants:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= warmup:
                times[name].append(e0.elapsed_time(e1))
    return times


def as_int32(t):
    """the decoded unsigned elements as int32 (through the signed view and a mask where torch converts no unsigned tensor of this width)"""
    try:
        return t.to(torch.int32)
    except (RuntimeError, TypeError):
        signed = t.view(torch.int16 if t.element_size() == 2 else torch.int8).to(torch.int32)
        return signed & ((1 << (8 * t.element_size())) - 1)


def bench_config(name, dev, steps, stream, cases, extras):
    """cases: [(label, forms, lag_forms, dtype, torch route f(rows int-convertible [G, D]) -> [G, K])]"""
    (codec, esz, D, chunk_len, nchunks), x = bench_input(name, dev)
    cd = sz.ChunkedCodec(codec, esz, D, chunk_len, device=dev)
    batch = cd.compress(x)
    del x
    cid = _lib.CODEC_DELTA if codec == "delta" else _lib.CODEC_XFF
    ne = nchunks * chunk_len
    G = ne // D
    dec = torch.empty(ne, dtype=cd.dtype, device=dev)
    shape = {"config": name, "codec": codec, "elem_bytes": esz, "ndims": D, "chunk_len": chunk_len, "nchunks": nchunks}

    def run_dec():
        cd.decompress_into(batch.data, batch.offsets, nchunks, dec)

    variants = [("decompress", run_dec)]
    info = {"decompress": dict(what="decompress", out_bytes=ne * esz), "decompress_again": dict(what="decompress", again=True, out_bytes=ne * esz)}
    keep, bad = [], False
    if extras:
        # the linear filter with the form a - b (one bit a row out), and project rows to float32 at K = 1 and 2 (the same bytes out)
        w, _, bias, lo, hi = rowops.linear_terms({0: 1, 1: -1}, None, 0, 1, None, D, esz, dev)
        mask = torch.empty((nchunks, (chunk_len // D + 7) // 8), dtype=torch.uint8, device=dev)
        counts = torch.empty(nchunks, dtype=torch.int32, device=dev)

        def run_filter():
            _lib.check(_lib.filter_linear(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, w.data_ptr(), None, bias, lo, hi, 0,
                                          None, mask.data_ptr(), counts.data_ptr(), None, stream()))
        variants.append(("filter_linear", run_filter))
        info["filter_linear"] = dict(what="filter_linear", form="a - b >= 1", out_bytes=mask.numel() + counts.numel() * 4)
        for K in (1, 2):
            slots = rowops.project_slots(list(range(K)), D, dev)
            pout = torch.empty(G * K, dtype=torch.float32, device=dev)

            def run_proj(slots=slots, pout=pout, K=K):
                _lib.check(_lib.project_rows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, slots.data_ptr(), K, _lib.PROJECT_F32,
                                             None, None, 0, pout.data_ptr(), None, stream()))
            variants.append((f"project_float32_K{K}", run_proj))
            info[f"project_float32_K{K}"] = dict(what="project_float32", ncolumns=K, out_bytes=pout.numel() * 4)
            keep.append(pout)
    pairs = []
    for label, forms, lag_forms, dtype, route in cases:
        wt, ut, bt = rowops.derive_forms(forms, lag_forms, 0, D, esz, dev)
        K = wt.shape[0]
        flt = dtype != torch.int32
        out = torch.empty(G * K, dtype=dtype, device=dev)
        scale = torch.linspace(0.5, 2.0, K, device=dev) if flt else None
        offset = torch.linspace(-3.0, 3.0, K, device=dev) if flt else None
        tmp = torch.empty(max(_lib.derive_rows_tmp_bytes(esz, nchunks, D) // 8, 1), dtype=torch.int64, device=dev) if ut is not None else None
        fmt = _lib.DERIVE_F32 if flt else _lib.DERIVE_I32
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731

        def run_derive(wt=wt, ut=ut, bt=bt, K=K, out=out, scale=scale, offset=offset, tmp=tmp, fmt=fmt):
            _lib.check(_lib.derive_rows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, K, wt.data_ptr(), ptr(ut), bt.data_ptr(), fmt,
                                        ptr(scale), ptr(offset), None, 0, ptr(tmp), out.data_ptr(), None, stream()))

        def run_torch(route=route, scale=scale, offset=offset, flt=flt):
            run_dec()
            s = route(dec.view(G, D))
            return s.to(torch.float32) * scale + offset if flt else s

        before = _lib.dispatch_counts()
        run_derive()
        after = _lib.dispatch_counts()
        want = run_torch()
        torch.cuda.synchronize()
        ok = bool(tuple(want.shape) == (G, K) and want.dtype == dtype and torch.equal(out.view(torch.int32), want.contiguous().view(-1).view(torch.int32)))
        del want
        bad = bad or not ok
        info[f"derive_{label}"] = dict(what="derive_rows", case=label, nforms=K, lag=ut is not None, dtype=str(dtype).split(".")[-1],
                                       family=[k for k in after if after[k] != before[k]], ok=ok, out_bytes=out.numel() * 4)
        info[f"torch_{label}"] = dict(what="decompress + torch expression", case=label, out_bytes=out.numel() * 4)
        variants += [(f"derive_{label}", run_derive), (f"torch_{label}", run_torch)]
        pairs.append(label)
        keep.append(out)
    variants.append(("decompress_again", run_dec))
    times = time_rounds(variants, steps)
    for label in pairs:
        info[f"derive_{label}"]["beats_torch"] = bool(statistics.median(times[f"derive_{label}"]) < min(times[f"torch_{label}"]))
    lines = []
    for key, _ in variants:
        t = times[key]
        lines.append(dict(shape, variant=key, **info[key], ms=round(statistics.median(t), 4), ms_min=round(min(t), 4), ms_max=round(max(t), 4)))
        print(json.dumps(lines[-1]), flush=True)
    return lines, bad


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

    def spread(v):
        return (as_int32(v[:, 0]) - as_int32(v[:, 1])).unsqueeze(1)

    def two(v):
        return torch.stack([as_int32(v[:, 0]) - as_int32(v[:, 1]), as_int32(v[:, 2]) + as_int32(v[:, 3])], dim=1)

    def diff(v):
        r = as_int32(v)
        return torch.diff(r, dim=0, prepend=r[:1])

    headline = [("a_minus_b_int32", [{0: 1, 1: -1}], None, torch.int32, spread),
                ("a_minus_b_float32", [{0: 1, 1: -1}], None, torch.float32, spread),
                ("K2_float32", [{0: 1, 1: -1}, {2: 1, 3: 1}], None, torch.float32, two),
                ("diff8_int32", [{c: 1} for c in range(8)], [{c: -1} for c in range(8)], torch.int32, diff)]
    wide = [("K2_int32", [{0: 1, 1: -1}, {2: 1, 3: 1}], None, torch.int32, two)]
    lines, bad = [], False
    for name, cases, extras in (("cfg2", headline, True), ("cfg3_10k", wide, False)):
        got, b = bench_config(name, dev, args.steps, stream, cases, extras)
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
