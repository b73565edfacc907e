"""Windowed query against decompress + torch, on the bench's own inputs (tests/test_gpu_bench_data.py: bench_input).

For cfg2 (u16 x 8, FIRE), cfg3_10k (u8 x 80, delta) and cfg1 (u8 x 1, delta) at window_rows 8, 64 and R (a chunk's rows):
  (a) sprintz_mi355x_query_windows, min + max + sum, reduce only (nothing but the results leaves the chip)
  (b) decompress_into + the cheapest torch reductions that give the same three results
  (c) the per-chunk query_batch sum, reduce only: the floor
Device events, warm-up, `--steps` timed launches per measurement; (a) and (b) alternate in one process, `--repeats` times,
and the spread of the repeats is reported.  (a) is checked against (b) once per shape.
  python tools/bench_query_windows.py [--steps 20] [--repeats 3] [--families default,nofast] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import sprintz_amd as sz  # noqa: E402
from sprintz_amd import _lib  # noqa: E402
from synth import synth_torch  # noqa: E402

CONFIGS = {   # what bench.py generates for these configurations (rank 0 of 1)
    "cfg2": (("xff", 2, 8, 5120, 131072), ("walk", 2, 131072, 640, 8, 8)),
    "cfg3_10k": (("delta", 1, 80, 10240, 52429), ("walk", 1, 52429, 128, 80, 2)),
    "cfg1": (("delta", 1, 1, 1024, 524288), ("walk", 1, 524288, 1024, 1, 2)),
}


def timed(fn, steps, warmup=3):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--configs", default="cfg2,cfg3_10k,cfg1")
    ap.add_argument("--windows", default="8,64,R")
    ap.add_argument("--families", default="default", help="default and / or nofast (SPRINTZ_OPT_NO_FAST: decode_kernel.h)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    lines = []
    for name in args.configs.split(","):
        (codec, esz, D, chunk_len, nchunks), (kind, _, _, rows, _, step) = CONFIGS[name]
        x = synth_torch(kind, esz, nchunks, rows, D, dev, seed=123, step=step, chunk0=0)
        cd = sz.ChunkedCodec(codec, esz, D, chunk_len, device=dev)
        batch = cd.compress(x)
        del x
        cid = _lib.CODEC_DELTA if codec == "delta" else _lib.CODEC_XFF
        R = chunk_len // D
        out = torch.empty(nchunks * chunk_len, dtype=cd.dtype, device=dev)
        partials = torch.empty((nchunks, D), dtype=torch.int64, device=dev)
        dec_bytes = nchunks * chunk_len * esz

        def floor_c():
            _lib.check(_lib.query_batch(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, 2, 0, 0,
                                        None, partials.data_ptr(), None, stream()))
        for wtxt in args.windows.split(","):
            W = R if wtxt == "R" else int(wtxt)
            nwin = -(-R // W)
            mn = torch.empty((nchunks, nwin, D), dtype=cd.dtype, device=dev)
            mx = torch.empty_like(mn)
            sm = torch.empty((nchunks, nwin, D), dtype=torch.int64, device=dev)

            def run_a():
                _lib.check(_lib.query_windows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, W, 7, 0,
                                              mn.data_ptr(), mx.data_ptr(), sm.data_ptr(), None, stream()))

            def run_b():
                cd.decompress_into(batch.data, batch.offsets, nchunks, out)
                v = out.view(nchunks, nwin, W, D)
                if esz == 1:                     # torch reduces uint8 natively
                    return v.amin(dim=2), v.amax(dim=2), v.sum(dim=2, dtype=torch.int64)
                v32 = v.to(torch.int32)          # uint16 has no amin / amax in torch: one widening pass
                return v32.amin(dim=2), v32.amax(dim=2), v32.sum(dim=2, dtype=torch.int64)
            for fam in args.families.split(","):
                _lib.check(_lib.set_option(_lib.OPT_NO_FAST, 1 if fam == "nofast" else 0))
                run_a()
                ref = run_b()
                torch.cuda.synchronize()
                ok = bool(torch.equal(mn.to(torch.int32), ref[0].to(torch.int32)) and torch.equal(mx.to(torch.int32), ref[1].to(torch.int32))
                          and torch.equal(sm, ref[2]))
                del ref
                ta, tb = [], []
                for _ in range(args.repeats):
                    ta.append(timed(run_a, args.steps))
                    tb.append(timed(run_b, args.steps))
                tc = timed(floor_c, args.steps)
                rec = {"config": name, "family": fam, "window_rows": W, "nwin": nwin, "ok": ok,
                       "a_query_windows_ms": [round(t, 4) for t in ta], "b_decompress_torch_ms": [round(t, 4) for t in tb],
                       "c_query_batch_sum_ms": round(tc, 4),
                       "a_min_ms": round(min(ta), 4), "b_min_ms": round(min(tb), 4),
                       "a_spread_pct": round(100 * (max(ta) - min(ta)) / min(ta), 2),
                       "b_spread_pct": round(100 * (max(tb) - min(tb)) / min(tb), 2),
                       "b_over_a": round(min(tb) / min(ta), 3),
                       "out_bytes_per_decoded_byte": round(nchunks * nwin * D * (2 * esz + 8) / dec_bytes, 4)}
                print(json.dumps(rec), flush=True)
                lines.append(rec)
            del mn, mx, sm
        _lib.set_option(_lib.OPT_NO_FAST, 0)
        del out, partials, batch, cd
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
