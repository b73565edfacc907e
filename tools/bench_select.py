"""Select rows against its alternatives, on the bench's headline input (tests/test_gpu_bench_data.py: bench_input("cfg2")).

Two masks: the band predicate of tools/bench_filter.py (columns 0 and D - 1 inside their own quartiles, mode ALL: a quarter of the
rows) and a seeded Bernoulli mask with p = 1/64.  For each, the median of `--steps` single timings after warm-up:
  (a) ChunkedCodec.where() end to end: the filter launch, the prefix sum of its counts, the read of the total, the select launch
      (host clock around the call, device idle before and after).  The Bernoulli mask has no predicate: there it is select_rows(mask,
      counts) end to end -- where() without its filter launch.
  (b) the select launch alone (device events around sprintz_mi355x_select_rows)
  (c) decompress_into + the torch predicate + a boolean index, dec.view(-1, D)[ok]: what a caller does without (a); (c2) the same
      with `ok` given -- decompress + the index alone.  (For the Bernoulli mask `ok` is the mask unpacked once, outside the timing.)
  (d) the route without select_rows: filter_rows(ids=True) -- for the Bernoulli mask filter_row_ids -- then gather_rows(ids, 1), on the
      first `--slice-chunks` chunks; (a) is timed on that slice too.  `--full-route` times (d) once on the whole batch as well.
(a) is checked against (c) once per mask.  One JSON line per mask; `--out` writes them behind a line that names the device and the commit.
Exits non-zero where (a) differs from (c) or is not faster than (c) and than (d).
  python tools/bench_select.py [--steps 20] [--slice-chunks 2048] [--full-route] [--commit TEXT] [--out FILE]
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
    ap.add_argument("--slice-chunks", type=int, default=2048)
    ap.add_argument("--full-route", action="store_true")
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    head = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "commit": args.commit, "steps": args.steps,
            "slice_chunks": args.slice_chunks}
    print(json.dumps(head), flush=True)
    (codec, esz, D, chunk_len, nchunks), x = bench_input("cfg2", dev)
    cd = sz.ChunkedCodec(codec, esz, D, chunk_len, device=dev)
    batch = cd.compress(x)
    del x
    cid = _lib.CODEC_DELTA if codec == "delta" else _lib.CODEC_XFF
    R = chunk_len // D
    MB = -(-R // 8)
    assert R % 8 == 0
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

    ns = min(args.slice_chunks, nchunks)
    part = sz.CompressedBatch(batch.data, batch.offsets[: ns + 1].contiguous(), batch.sizes[:ns].contiguous(), ns, ns * chunk_len, chunk_len, D)
    weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(64)
    bern = (torch.rand(nchunks * R, generator=gen, device=dev) < 1.0 / 64)
    lines = []
    for name in ("band", "p=1/64"):
        if name == "band":
            f = cd.filter_rows(batch, lo, hi)
            mask, counts = f["mask"], f["counts"]
            ok_ref = predicate()
            run_a = lambda: cd.where(batch, lo, hi)                                   # noqa: E731
            run_a_part = lambda: cd.where(part, lo, hi)                               # noqa: E731
            run_d = lambda b: cd.gather_rows(b, cd.filter_rows(b, lo, hi, ids=True)["ids"], 1, check=False)   # noqa: E731

            def run_c():
                cd.decompress_into(batch.data, batch.offsets, nchunks, dec)
                return dec.view(view).view(-1, D)[predicate()]
        else:
            ok_ref = bern
            mask = (bern.view(-1, 8).to(torch.int32) * weights).sum(dim=1).to(torch.uint8).view(nchunks, MB)
            counts = bern.view(nchunks, R).sum(dim=1).to(torch.int32)
            run_a = lambda: cd.select_rows(batch, mask, counts, check=False)          # noqa: E731
            run_a_part = lambda: cd.select_rows(part, mask[:ns], counts[:ns], check=False)   # noqa: E731

            def run_d(b):
                n = b.nchunks
                c64 = counts[:n].to(torch.int64)
                incl = torch.cumsum(c64, 0)
                total = int(incl[-1].item())
                ids = torch.empty(total, dtype=torch.int64, device=dev)
                bases = (incl - c64).contiguous()
                _lib.check(_lib.filter_row_ids(mask.data_ptr(), bases.data_ptr(), n, chunk_len, D, ids.data_ptr(), total, stream()))
                return cd.gather_rows(b, ids, 1, check=False)

            def run_c():
                cd.decompress_into(batch.data, batch.offsets, nchunks, dec)
                return dec.view(view).view(-1, D)[ok_ref]

        def run_c2():
            cd.decompress_into(batch.data, batch.offsets, nchunks, dec)
            return dec.view(view).view(-1, D)[ok_ref]

        c64 = counts.to(torch.int64)
        incl = torch.cumsum(c64, 0)
        total = int(incl[-1].item())
        bases = (incl - c64).contiguous()
        rows = torch.empty(total * D, dtype=cd.dtype, device=dev)

        def run_b():
            _lib.check(_lib.select_rows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, mask.data_ptr(),
                                        bases.data_ptr(), total, 0, rows.data_ptr(), None, None, stream()))

        got = run_a()["rows"]
        want = run_c()
        run_b()
        torch.cuda.synchronize()
        ok = bool(total == int(ok_ref.sum().item()) and torch.equal(got.view(view), want.view(view)) and torch.equal(rows.view(view).view(-1, D), want.view(view)))
        ok_part = torch.equal(run_a_part()["rows"].view(view), run_d(part).view(view).view(-1, D))
        del got, want
        rec = {"mask": name, "codec": codec, "elem_bytes": esz, "ndims": D, "chunk_len": chunk_len, "nchunks": nchunks, "ok": ok and ok_part,
               "rows": nchunks * R, "rows_selected": total,
               "a_end_to_end_ms": median_ms(run_a, args.steps, host=True),
               "b_select_launch_ms": median_ms(run_b, args.steps),
               "c_decompress_predicate_index_ms": median_ms(run_c, args.steps, host=True),
               "c2_decompress_index_ms": median_ms(run_c2, args.steps, host=True),
               "slice_a_end_to_end_ms": median_ms(run_a_part, args.steps, host=True),
               "slice_d_ids_gather_ms": median_ms(lambda: run_d(part), min(args.steps, 5), warmup=1, host=True),
               "compressed_bytes": batch.total_bytes(), "decoded_bytes": nchunks * chunk_len * esz, "selected_bytes": total * D * esz}
        if args.full_route:
            rec["full_d_ids_gather_ms"] = median_ms(lambda: run_d(batch), 1, warmup=0, host=True)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del rows
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(head) + "\n")
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
    if not all(r["ok"] for r in lines):
        sys.exit("select_rows differs from decompress + torch, or from filter_row_ids + gather_rows")
    for r in lines:
        if r["a_end_to_end_ms"] >= r["c_decompress_predicate_index_ms"] or r["slice_a_end_to_end_ms"] >= r["slice_d_ids_gather_ms"]:
            sys.exit(f"{r['mask']}: where() is not faster than both alternatives")


if __name__ == "__main__":
    main()
