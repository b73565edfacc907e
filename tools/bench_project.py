"""Project rows against its alternatives, on the bench's headline input (tests/rowdata.py: bench_input("cfg2"): uint16 x 8, FIRE, 10 KB
chunks, 131 072 chunks) and on BASELINE config 3 at 10 KB (bench_input("cfg3_10k"): uint8 x 80, delta -- a shape the generic kernel serves).

Everything in one job, every variant of a shape timed in turn, round after round (`--steps` rounds behind 3 warm-up rounds), device events
around the work; a line gives the median, the fastest and the slowest round:
  decompress                     the plain decode's launch (decompress_into) -- twice a round, first and last, as the job's own spread
  float_rows_float32             the decode that writes twice the bytes
  project_raw / project_float32  the projection's launch on preallocated outputs, at K = 1, 2, 4 and 8 columns (the first K; K = 8: the identity)
  decompress_slice / float_rows_slice   the torch routes they replace: the full decode, then [:, :K].contiguous() -- the strided slice-copy, torch's
                                 cheapest form of [:, cols] (the decoded uint16 tensor is viewed as int16 for it: torch indexes no uint16 tensor)
The projection is checked against its torch route once per (format, K), exactly.  One JSON line per measurement; `--out` writes them behind a line
that names the device and the commit.  Exits non-zero where a result differs.
  python tools/bench_project.py [--steps 20] [--commit TEXT] [--out FILE]
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


def bench_config(name, dev, steps, stream, ks, floats):
    (codec, esz, D, chunk_len, nchunks), x = bench_input(name, dev)
    cd = sz.ChunkedCodec(codec, esz, D, chunk_len, device=dev)
    batch = cd.compress(x)
    del x
    cid = _lib.CODEC_DELTA if codec == "delta" else _lib.CODEC_XFF
    ne = nchunks * chunk_len
    G = ne // D
    dec = torch.empty(ne, dtype=cd.dtype, device=dev)
    dec_rows = dec.view(torch.int16 if esz == 2 else torch.int8).view(G, D)
    fdec = torch.empty(ne, dtype=torch.float32, device=dev) if floats else None
    scale = torch.linspace(0.5, 2.0, D, device=dev)
    offset = torch.linspace(-3.0, 3.0, D, device=dev)
    shape = {"config": name, "codec": codec, "elem_bytes": esz, "ndims": D, "chunk_len": chunk_len, "nchunks": nchunks}

    def run_dec():
        cd.decompress_into(batch.data, batch.offsets, nchunks, dec)

    def run_float():
        _lib.check(_lib.float_rows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, _lib.FLOAT_F32, scale.data_ptr(),
                                   offset.data_ptr(), 0, fdec.data_ptr(), None, stream()))

    variants = [("decompress", run_dec)]
    if floats:
        variants.append(("float_rows_float32", run_float))
    info, keep, bad = {}, [], False
    for K in ks:
        cols = list(range(K))
        slots = rowops.project_slots(cols, D, dev)
        for fmt, label in ((_lib.PROJECT_RAW, "raw"),) + (((_lib.PROJECT_F32, "float32"),) if floats else ()):
            raw = fmt == _lib.PROJECT_RAW
            out = torch.empty(G * K, dtype=cd.dtype if raw else torch.float32, device=dev)
            sc, of = (None, None) if raw else (scale[:K].contiguous(), offset[:K].contiguous())

            def run_proj(slots=slots, out=out, sc=sc, of=of, fmt=fmt, K=K):
                _lib.check(_lib.project_rows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, slots.data_ptr(), K, fmt,
                                             sc.data_ptr() if sc is not None else None, of.data_ptr() if of is not None else None, 0, out.data_ptr(), None, stream()))

            def run_slice(raw=raw, K=K):
                if raw:
                    run_dec()
                    return dec_rows[:, :K].contiguous()
                run_float()
                return fdec.view(G, D)[:, :K].contiguous()

            before = _lib.dispatch_counts()
            run_proj()
            after = _lib.dispatch_counts()
            want = run_slice()
            torch.cuda.synchronize()
            view = (torch.int16 if esz == 2 else torch.int8) if raw else torch.int32
            ok = bool(torch.equal(out.view(view), want.reshape(-1).view(view)))
            del want
            bad = bad or not ok
            key = f"project_{label}_K{K}"
            info[key] = dict(what=f"project_{label}", ncolumns=K, family=[k for k in after if after[k] != before[k]], ok=ok, out_bytes=out.numel() * out.element_size())
            info[f"{'decompress' if raw else 'float_rows'}_slice_K{K}"] = dict(what=f"{'decompress' if raw else 'float_rows'}_slice", ncolumns=K,
                                                                                 out_bytes=out.numel() * out.element_size())
            variants += [(key, run_proj), (f"{'decompress' if raw else 'float_rows'}_slice_K{K}", run_slice)]
            keep.append(out)
    variants.append(("decompress_again", run_dec))
    info["decompress"] = dict(what="decompress", out_bytes=ne * esz)
    info["decompress_again"] = dict(what="decompress", again=True, out_bytes=ne * esz)
    info["float_rows_float32"] = dict(what="float_rows_float32", out_bytes=ne * 4)
    times = time_rounds(variants, steps)
    lines = []
    for key, _ in variants:
        t = times[key]
        lines.append(dict(shape, **info[key], ms=round(statistics.median(t), 4), ms_min=round(min(t), 4), ms_max=round(max(t), 4)))
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
    lines, bad = [], False
    for name, ks, floats in (("cfg2", (1, 2, 4, 8), True), ("cfg3_10k", (4,), False)):
        got, b = bench_config(name, dev, args.steps, stream, ks, floats)
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
