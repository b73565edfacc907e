"""Segment rows against its alternatives, on the bench's headline input (tests/test_gpu_bench_data.py: bench_input("cfg2")) and on a
constant batch of the same shape under the delta codec.

The mask is the band predicate of tools/bench_aggregate.py (columns 0 and D - 1 inside their own quartiles, mode ALL: a quarter of the
rows, in spans) as filter_rows writes it.  For both rules (runs, splits), the median of `--steps` single timings after 3 warm-up calls:
  (s) the segment_rows launch alone, all five ops, the bases the prefix sum of segment_count (device events around the call)
  (c) the segment_count launch
  (e) ChunkedCodec.segment_rows end to end: count, prefix sum, one read of the total, the launch and the fold (host clock)
  (a) the aggregate_rows launch of the same batch and mask at one window a chunk, all four ops: the same decode with fixed edges
  (d) the route through the decoded batch: decompress_into + the mask's diff + cumsum for segment ids + scatter_reduce a output (host clock)
(s) is checked against (d) once per rule.  The constant batch gives (s) and (a) alone: nearly all of a chunk is delta runs, which (s)
crosses in O(1) where their mask bytes hold no edge -- time a library built with -DSPRINTZ_SEG_RUN_SHORTCUT=0 through
SPRINTZ_MI355X_LIB for the other side.  One JSON line per (batch, rule); `--out` writes them behind a line that names the device and
the commit.  Exits non-zero where (s) differs from (d).
  python tools/bench_segments.py [--steps 20] [--commit TEXT] [--label TEXT] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import sprintz_amd as sz  # noqa: E402
from sprintz_amd import _lib  # noqa: E402
from bench_aggregate import median_ms  # noqa: E402
from rowdata import bench_input


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    head = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "commit": args.commit, "steps": args.steps, "label": args.label,
            "lib": os.path.basename(_lib.LIB_PATH)}
    print(json.dumps(head), flush=True)
    (codec, esz, D, chunk_len, nchunks), x = bench_input("cfg2", dev)
    R = chunk_len // D
    MB = -(-R // 8)
    assert R % 8 == 0
    top = (1 << (8 * esz)) - 1
    view = torch.int16 if esz == 2 else torch.int8
    i64 = dict(dtype=torch.int64, device=dev)
    lines = []
    mask = None
    for label in ("headline", "constant, delta"):
        if label == "headline":
            cd = sz.ChunkedCodec(codec, esz, D, chunk_len, device=dev)
        else:
            cd = sz.ChunkedCodec("delta", esz, D, chunk_len, device=dev)
            x.view(view).fill_(0x1234 if esz == 2 else 0x25)
        batch = cd.compress(x)
        cid = _lib.CODEC_DELTA if cd.codec == "delta" else _lib.CODEC_XFF
        dec = torch.empty(nchunks * chunk_len, dtype=cd.dtype, device=dev)
        cd.decompress_into(batch.data, batch.offsets, nchunks, dec)
        if mask is None:                                                 # the band of the headline batch, for both batches
            lo, hi = [0] * D, [top] * D
            for d in sorted({0, D - 1}):
                col = dec.view(view).view(-1, D)[:, d].to(torch.int32) & top
                lo[d] = int(torch.kthvalue(col, int(0.25 * (col.numel() - 1)) + 1).values.item())
                hi[d] = int(torch.kthvalue(col, int(0.75 * (col.numel() - 1)) + 1).values.item())
                del col
            f = cd.filter_rows(batch, lo, hi)
            mask = f["mask"].contiguous()
            selected = int(f["counts"].sum().item())
            bit = torch.arange(8, device=dev, dtype=torch.int32)
            ok = ((mask.view(-1, 1).to(torch.int32) >> bit) & 1).bool().view(nchunks, R)     # the mask as one bool a row
        lens = torch.full((nchunks,), chunk_len, **i64)
        for mode, mname in ((_lib.SEG_RUNS, "runs"), (_lib.SEG_SPLITS, "splits")):
            counts = torch.empty(nchunks, dtype=torch.int32, device=dev)

            def run_c():
                _lib.check(_lib.segment_count(mask.data_ptr(), nchunks, chunk_len, D, mode, lens.data_ptr(), counts.data_ptr(), stream()))
            run_c()
            c64 = counts.to(torch.int64)
            bases = (torch.cumsum(c64, 0) - c64).contiguous()
            S = int(c64.sum().item())
            mn = torch.empty(S * D, dtype=cd.dtype, device=dev)
            mx = torch.empty(S * D, dtype=cd.dtype, device=dev)
            sm = torch.empty(S * D, **i64)
            rows = torch.empty(S, dtype=torch.int32, device=dev)
            start = torch.empty(S, **i64)
            amn = torch.empty(nchunks * D, dtype=cd.dtype, device=dev)
            amx = torch.empty(nchunks * D, dtype=cd.dtype, device=dev)
            asm = torch.empty(nchunks * D, **i64)
            acnt = torch.empty(nchunks, dtype=torch.int32, device=dev)

            def run_s():
                _lib.check(_lib.segment_rows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, mask.data_ptr(), mode,
                                             bases.data_ptr(), S, 31, 0, mn.data_ptr(), mx.data_ptr(), sm.data_ptr(), rows.data_ptr(), start.data_ptr(), None, stream()))

            def run_a():
                _lib.check(_lib.aggregate_rows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, mask.data_ptr(), R, 15, 0,
                                               amn.data_ptr(), amx.data_ptr(), asm.data_ptr(), acnt.data_ptr(), None, stream()))

            def run_e():
                return cd.segment_rows(batch, mask, mode=mname, check=False)

            def run_d():
                cd.decompress_into(batch.data, batch.offsets, nchunks, dec)
                v = dec.view(view).to(torch.int32).view(-1, D) & top
                if mode == _lib.SEG_RUNS:
                    prev = torch.cat([torch.zeros((nchunks, 1), dtype=torch.bool, device=dev), ok[:, :-1]], dim=1)
                    st = (ok & ~prev).view(-1)
                    member = ok.view(-1)
                else:
                    st = ok.clone()
                    st[:, 0] = True
                    st = st.view(-1)
                    member = None
                ids = torch.cumsum(st.to(torch.int64), 0) - 1
                n = int(ids[-1].item()) + 1
                if member is not None:
                    ids, v = ids[member], v[member]
                idx = ids.view(-1, 1).expand(-1, D)
                o_mn = torch.full((n, D), top, dtype=torch.int32, device=dev).scatter_reduce_(0, idx, v, "amin")
                o_mx = torch.zeros((n, D), dtype=torch.int32, device=dev).scatter_reduce_(0, idx, v, "amax")
                o_sm = torch.zeros((n, D), **i64).scatter_add_(0, idx, v.to(torch.int64))
                o_rows = torch.bincount(ids, minlength=n)
                o_start = st.nonzero().view(-1)
                return o_mn, o_mx, o_sm, o_rows, o_start

            run_s()
            torch.cuda.synchronize()
            got = (mn.view(view).to(torch.int32).view(-1, D) & top, mx.view(view).to(torch.int32).view(-1, D) & top, sm.view(-1, D), rows.to(torch.int64), start)
            want = run_d()
            okay = all(g.shape == w.shape and torch.equal(g, w.to(g.dtype)) for g, w in zip(got, want))
            del want
            rec = {"batch": label, "rule": mname, "codec": cd.codec, "elem_bytes": esz, "ndims": D, "chunk_len": chunk_len, "nchunks": nchunks, "ok": bool(okay),
                   "rows": nchunks * R, "rows_selected": selected, "segments": S,
                   "s_segment_launch_ms": median_ms(run_s, args.steps),
                   "a_aggregate_launch_ms": median_ms(run_a, args.steps)}
            if label == "headline":
                rec.update({"c_segment_count_ms": median_ms(run_c, args.steps),
                            "e_segment_rows_end_to_end_ms": median_ms(run_e, args.steps, host=True),
                            "d_decompress_torch_ms": median_ms(run_d, args.steps, host=True)})
            rec.update({"compressed_bytes": batch.total_bytes(), "decoded_bytes": nchunks * chunk_len * esz, "mask_bytes": nchunks * MB,
                        "output_bytes": S * (D * (2 * esz + 8) + 12)})
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del mn, mx, sm, rows, start
        del dec, batch
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(head) + "\n")
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
    if not all(r["ok"] for r in lines):
        sys.exit("segment_rows differs from decompress + torch")


if __name__ == "__main__":
    main()
