"""Zone-map pruning against the unpruned filter on the bench's headline input (tests/test_gpu_bench_data.py: bench_input("cfg2"), u16 x 8,
FIRE, 131 072 chunks), all in one job.  For each predicate -- a band on column 0 between two of the column's quantiles, mode ALL, the other
columns unconstrained -- the median of `--steps` timings after 3 warm-ups of
  (f)  sprintz_mi355x_filter_rows on the whole container, mask + counts: the unpruned launch
  (z)  the zoned call end to end: sprintz_mi355x_zone_prune_box, the 8-byte read of the survivor count, filter_rows on the survivors'
       offsets into compact buffers, sprintz_mi355x_zone_expand -- device events around all of it (the read-back's wait lies between them),
       and the same by the host's clock around a synchronise
  (p)  the prune launches alone (classify, size scan, compact)
  (e)  the expand launch alone
and sprintz_mi355x_zone_map once (median of 5).  (z)'s mask and counts are checked against (f)'s, bit for bit.

How many chunks survive.  The headline's chunks each start at a level of their own, uniform over the 16 bits, and then walk by +-8 for
640 rows: a chunk's zone is a few hundred values wide, so a band on one column is straddled by about one chunk in a hundred whichever
quantiles bound it -- the chunks inside and outside it are decided by their zone.  That is the tool's "natural" point.  The other
points of the curve -- about 10 %, 50 %, 75 %, 90 % and 100 % of the chunks surviving -- are reached with the same band by WIDENING the zone of a
random subset of the chunks to the column's whole range: a wider zone is still a sound zone (the result stays exact, and is checked), it
only proves less, which is what a coarser or staler map would do.  0 % is the band 0 .. 0xFFFF: every chunk is ALL.

  python tools/bench_zone_prune.py [--steps 20] [--commit TEXT] [--out FILE]
prints its record -- the hypothesis first, then one JSON line per predicate and the derived figures -- and with --out writes it to FILE.
profiles/zone_prune.txt holds such a record under a summary and a verdict written by hand."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sprintz_amd as sz  # noqa: E402
from sprintz_amd import _lib  # noqa: E402
from rowdata import bench_input

HYPOTHESIS = """Hypothesis, written before the first run: a filter's time is its decode, chunk by chunk, so with a zone map the zoned call (z) falls
about in proportion to the chunks that survive, plus a constant for the prune launches, the 8-byte read-back and the expand launch that
is measured in microseconds, not in tenths of a millisecond:  z(s) ~ s * f + k,  s the surviving fraction, f the unpruned launch."""


def timed(fn, steps, warmup=3):
    """-> (median ms between device events around fn, median ms by the host's clock around fn and a synchronise)"""
    for _ in range(warmup):
        fn()
    ev, wall = [], []
    for _ in range(steps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(e0.elapsed_time(e1))
    return round(statistics.median(ev), 4), round(statistics.median(wall), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    head = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "commit": args.commit, "steps": args.steps,
            "lib": os.path.basename(_lib.LIB_PATH)}
    print(HYPOTHESIS + "\n", flush=True)
    print(json.dumps(head), flush=True)
    (codec, esz, D, chunk_len, n), x = bench_input("cfg2", dev)
    R, top = chunk_len // D, (1 << (8 * esz)) - 1
    MB = R // 8
    cd = sz.ChunkedCodec(codec, esz, D, chunk_len, device=dev)
    batch = cd.compress(x)
    cid = _lib.CODEC_DELTA if codec == "delta" else _lib.CODEC_XFF
    col = x.view(-1, D)[:, 0].to(torch.int32)
    q = {p: int(torch.kthvalue(col, int(p * (col.numel() - 1)) + 1).values.item()) for p in (0.25, 0.75)}
    del col, x
    zones = cd.zone_map(batch)
    zone_map_ms = timed(lambda: _lib.check(_lib.zone_map(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), n, chunk_len, D, 0,
                                                         zones.min.data_ptr(), zones.max.data_ptr(), zones.len.data_ptr(), stream())), 5)[0]
    width = (zones.max[:, 0].to(torch.int32) - zones.min[:, 0].to(torch.int32)).to(torch.float64)
    head2 = {"config": "cfg2", "codec": codec, "elem_bytes": esz, "ndims": D, "chunk_len": chunk_len, "nchunks": n, "compressed_bytes": batch.total_bytes(),
             "mask_bytes": n * MB, "zone_map_ms": zone_map_ms, "zone_bytes": 2 * n * D * esz + 8 * n,
             "column0_zone_width_median": float(width.median().item()), "column0_q25": q[0.25], "column0_q75": q[0.75],
             "prune_tmp_bytes": int(_lib.zone_prune_tmp_bytes(n))}
    print(json.dumps(head2), flush=True)

    mask = torch.empty((n, MB), dtype=torch.uint8, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    zmask = torch.empty((n, MB), dtype=torch.uint8, device=dev)
    zcounts = torch.empty(n, dtype=torch.int32, device=dev)
    cmask = torch.empty((n, MB), dtype=torch.uint8, device=dev)      # compact buffers at their largest: the tool times the library, not the allocator
    ccounts = torch.empty(n, dtype=torch.int32, device=dev)
    cls = torch.empty(n, dtype=torch.uint8, device=dev)
    pos = torch.empty(n + 1, dtype=torch.int64, device=dev)
    surv = torch.empty(n + 1, dtype=torch.int64, device=dev)
    tmp = torch.empty(_lib.zone_prune_tmp_bytes(n) // 8, dtype=torch.int64, device=dev)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(1)
    order = torch.randperm(n, generator=gen).to(dev)                 # which chunks lose their zone first

    def bounds(lo0, hi0):
        lo, hi = [0] * D, [top] * D
        lo[0], hi[0] = lo0, hi0
        as_t = lambda v: torch.tensor(v, dtype=torch.int32, device=dev).to(cd.dtype)      # noqa: E731
        return as_t(lo), as_t(hi)

    recs = []
    band = (q[0.25], q[0.75])
    for label, (lo0, hi0), widen in (("0 %: the band 0 .. top, every chunk ALL", (0, top), 0.0), ("natural: q25 .. q75 of column 0", band, 0.0),
                                     ("10 %", band, 0.10), ("50 %", band, 0.50), ("75 %", band, 0.75), ("90 %", band, 0.90),
                                     ("100 %", band, 1.0)):
        lo_t, hi_t = bounds(lo0, hi0)
        zmin, zmax = zones.min.clone(), zones.max.clone()
        k = int(round(widen * n))
        if k:                                                         # a wider zone proves less and stays sound
            zmin.view(torch.int16)[order[:k], 0] = 0
            zmax.view(torch.int16)[order[:k], 0] = -1                 # 0xFFFF

        def unpruned():
            _lib.check(_lib.filter_rows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), n, chunk_len, D, lo_t.data_ptr(), hi_t.data_ptr(),
                                        _lib.FILTER_ALL, 0, mask.data_ptr(), counts.data_ptr(), None, stream()))

        def prune():
            _lib.check(_lib.zone_prune_box(esz, n, chunk_len, D, batch.offsets.data_ptr(), zmin.data_ptr(), zmax.data_ptr(), zones.len.data_ptr(),
                                           lo_t.data_ptr(), hi_t.data_ptr(), _lib.FILTER_ALL, cls.data_ptr(), pos.data_ptr(), surv.data_ptr(),
                                           tmp.data_ptr(), stream()))

        def expand():
            _lib.check(_lib.zone_expand(n, chunk_len, D, cls.data_ptr(), pos.data_ptr(), zones.len.data_ptr(), cmask.data_ptr(), ccounts.data_ptr(),
                                        None, zmask.data_ptr(), zcounts.data_ptr(), None, stream()))

        def zoned():
            prune()
            ns = int(pos[n].item())
            if ns == n:
                _lib.check(_lib.filter_rows(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), n, chunk_len, D, lo_t.data_ptr(), hi_t.data_ptr(),
                                            _lib.FILTER_ALL, 0, zmask.data_ptr(), zcounts.data_ptr(), None, stream()))
                return ns
            if ns:
                _lib.check(_lib.filter_rows(cid, esz, batch.data.data_ptr(), surv.data_ptr(), ns, chunk_len, D, lo_t.data_ptr(), hi_t.data_ptr(),
                                            _lib.FILTER_ALL, 0, cmask.data_ptr(), ccounts.data_ptr(), None, stream()))
            expand()
            return ns

        unpruned()
        zmask.fill_(0x5A)
        zcounts.fill_(-7)
        ns = zoned()
        torch.cuda.synchronize()
        ok = bool(torch.equal(mask, zmask) and torch.equal(counts, zcounts))
        c = cls.to(torch.int64)
        rec = {"predicate": label, "lo0": lo0, "hi0": hi0, "zones_widened": k, "survivors": ns, "survivor_fraction": round(ns / n, 5),
               "none": int((c == 0).sum().item()), "all": int((c == 1).sum().item()), "rows_matching": int(counts.to(torch.int64).sum().item()), "ok": ok}
        rec["f_unpruned_ms"] = timed(unpruned, args.steps)[0]
        rec["z_zoned_ms"], rec["z_zoned_wall_ms"] = timed(zoned, args.steps)
        rec["p_prune_ms"] = timed(prune, args.steps)[0]
        rec["e_expand_ms"] = timed(expand, args.steps)[0]
        rec["z_over_f"] = round(rec["z_zoned_ms"] / rec["f_unpruned_ms"], 3)
        print(json.dumps(rec), flush=True)
        recs.append(rec)

    # the derived figures the issue asks for
    by = {r["predicate"].split(":")[0]: r for r in recs}
    full, tenth = by["100 %"], by["10 %"]
    derived = {"z_minus_f_at_100pct_ms": round(full["z_zoned_ms"] - full["f_unpruned_ms"], 4), "z_over_f_at_10pct": tenth["z_over_f"]}
    pts = sorted((r["survivor_fraction"], r["z_zoned_ms"] - r["f_unpruned_ms"]) for r in recs if r["survivors"] < n)
    derived["break_even_survivor_fraction"] = None                   # where z - f changes sign among the pruned points, linearly between them
    for (s0, d0), (s1, d1) in zip(pts, pts[1:]):
        if d0 <= 0 < d1:
            derived["break_even_survivor_fraction"] = round(s0 + (s1 - s0) * (0 - d0) / (d1 - d0), 3)
    if pts and pts[-1][1] <= 0:
        derived["break_even_survivor_fraction"] = f"above {pts[-1][0]}: the zoned call is faster at every pruned point measured"
    f_med = statistics.median(r["f_unpruned_ms"] for r in recs)
    derived["constant_ms_at_0pct"] = by["0 %"]["z_zoned_ms"]
    derived["fit"] = [{"survivor_fraction": r["survivor_fraction"], "z_ms": r["z_zoned_ms"],
                       "s_times_f_plus_constant_ms": round(r["survivor_fraction"] * f_med + by["0 %"]["z_zoned_ms"], 4)} for r in recs]
    print(json.dumps(derived), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(HYPOTHESIS + "\n\n")
            f.write(json.dumps(head) + "\n" + json.dumps(head2) + "\n")
            for rec in recs:
                f.write(json.dumps(rec) + "\n")
            f.write(json.dumps(derived) + "\n")
    if not all(r["ok"] for r in recs):
        sys.exit("the zoned call differs from the unpruned one")


if __name__ == "__main__":
    main()
