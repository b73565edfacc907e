"""Linear filter rows against filter rows, the windowed query and decompress + torch, on the bench's headline input
(tests/test_gpu_bench_data.py: bench_input("cfg2"), u16 x 8, FIRE), all in one job:
  (l)  sprintz_mi355x_filter_linear without a lag term: a - b >= 1, columns 0 and D - 1 ("WHERE a > b"), mask + counts
  (c)  ... with one: x[g, 0] - x[g - 1, 0] >= t (ChunkedCodec.filter_change's weights), the seam pass included
  (f)  sprintz_mi355x_filter_rows, the band predicate of tools/bench_filter.py: the reference
  (q)  sprintz_mi355x_query_windows, W = 64, min + max + sum: the floor
  (dl) decompress_into + the torch form of (l);  (dc) decompress_into + the torch form of (c)
and, on a constant batch of the same shape under the delta codec (one run a chunk), (l) and (c) again: the run shortcut's case.  Run it
once more with SPRINTZ_MI355X_LIB naming a library built with -DSPRINTZ_LIN_RUN_SHORTCUT=0 for the other half of that A/B.
The seam pass alone is a kernel of its own: a kernel trace of `--only c` names it (linear_seam_kernel).
Median of `--steps` launches after 3 warm-ups, device events around each launch.  (l) and (c) are checked against (dl) and (dc) once.
  python tools/bench_filter_linear.py [--steps 20] [--only l,c,f,q,dl,dc,const] [--commit TEXT] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sprintz_amd as sz  # noqa: E402
from sprintz_amd import _lib  # noqa: E402
from rowdata import bench_input


def median_ms(fn, steps, warmup=3):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(steps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return round(statistics.median(times), 4)


def pack_mask(match, nchunks, R):
    """bool [nchunks * R] -> uint8 [nchunks, R / 8] in filter rows' layout (R % 8 == 0)"""
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32, device=match.device)
    return (match.view(-1, 8).to(torch.int32) * w).sum(dim=1).to(torch.uint8).view(nchunks, R // 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--only", default="l,c,f,q,dl,dc,const")
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    only = set(args.only.split(","))
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    head = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "commit": args.commit, "steps": args.steps,
            "lib": os.path.basename(_lib.LIB_PATH)}
    print(json.dumps(head), flush=True)
    (codec, esz, D, chunk_len, nchunks), x = bench_input("cfg2", dev)
    R, top = chunk_len // D, (1 << (8 * esz)) - 1
    MB = R // 8
    t = 6                                                   # the change threshold: the walk steps by up to 8
    lines = []

    def measure(cname, data, label):
        cd = sz.ChunkedCodec(cname, esz, D, chunk_len, device=dev)
        batch = cd.compress(data)
        cid = _lib.CODEC_DELTA if cname == "delta" else _lib.CODEC_XFF
        mask = torch.empty((nchunks, MB), dtype=torch.uint8, device=dev)
        counts = torch.empty(nchunks, dtype=torch.int32, device=dev)
        tmp = torch.empty(_lib.filter_linear_tmp_bytes(esz, nchunks, D) // 8, dtype=torch.int64, device=dev)
        w_ab = torch.tensor([1] + [0] * (D - 2) + [-1], dtype=torch.int32, device=dev)
        w_c = torch.tensor([1] + [0] * (D - 1), dtype=torch.int32, device=dev)
        u_c = -w_c
        out = torch.empty(nchunks * chunk_len, dtype=cd.dtype, device=dev)

        def linear(w, u, lo):
            _lib.check(_lib.filter_linear(cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, w.data_ptr(),
                                          u.data_ptr() if u is not None else None, 0, lo, (1 << 31) - 1, 0, tmp.data_ptr() if u is not None else None,
                                          mask.data_ptr(), counts.data_ptr(), None, stream()))

        def torch_l():
            cd.decompress_into(batch.data, batch.offsets, nchunks, out)
            v = out.view(-1, D)
            return v[:, 0].to(torch.int32) > v[:, D - 1].to(torch.int32)

        def torch_c():
            cd.decompress_into(batch.data, batch.offsets, nchunks, out)
            a = out.view(-1, D)[:, 0].to(torch.int32)
            return torch.diff(a, prepend=a[:1]) >= t + 1

        rec = {"data": label, "codec": cname, "rows": nchunks * R, "compressed_bytes": batch.total_bytes(), "decoded_bytes": nchunks * chunk_len * esz,
               "mask_bytes": nchunks * MB, "tmp_bytes": tmp.numel() * 8}
        ok = True
        for key, run, ref in (("l", lambda: linear(w_ab, None, 1), torch_l), ("c", lambda: linear(w_c, u_c, t + 1), torch_c)):
            run()
            want = ref()
            torch.cuda.synchronize()
            good = bool(torch.equal(mask, pack_mask(want, nchunks, R)) and torch.equal(counts.to(torch.int64), want.view(nchunks, R).sum(dim=1)))
            rec[f"{key}_rows_matching"] = int(want.sum().item())
            rec[f"{key}_ok"] = good
            ok = ok and good
            del want
        rec["ok"] = ok
        if "l" in only:
            rec["l_filter_linear_a_gt_b_ms"] = median_ms(lambda: linear(w_ab, None, 1), args.steps)
        if "c" in only:
            rec["c_filter_change_with_seam_ms"] = median_ms(lambda: linear(w_c, u_c, t + 1), args.steps)
        if label == "walk":
            if "f" in only:
                dec = cd.decompress(batch).view(-1, D)
                lo, hi = [0] * D, [top] * D
                for d in sorted({0, D - 1}):               # the band: the column's own quartiles (tools/bench_filter.py)
                    col = dec[:, d].to(torch.int32)
                    lo[d] = int(torch.kthvalue(col, int(0.25 * (col.numel() - 1)) + 1).values.item())
                    hi[d] = int(torch.kthvalue(col, int(0.75 * (col.numel() - 1)) + 1).values.item())
                del dec, col
                lo_t = torch.tensor(lo, dtype=torch.int32, device=dev).to(cd.dtype)
                hi_t = torch.tensor(hi, dtype=torch.int32, device=dev).to(cd.dtype)
                rec["f_filter_rows_band_ms"] = median_ms(lambda: _lib.check(_lib.filter_rows(
                    cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, lo_t.data_ptr(), hi_t.data_ptr(), _lib.FILTER_ALL, 0,
                    mask.data_ptr(), counts.data_ptr(), None, stream())), args.steps)
            if "q" in only:
                nwin = -(-R // 64)
                mn = torch.empty((nchunks, nwin, D), dtype=cd.dtype, device=dev)
                mx = torch.empty_like(mn)
                sm = torch.empty((nchunks, nwin, D), dtype=torch.int64, device=dev)
                rec["q_query_windows_w64_ms"] = median_ms(lambda: _lib.check(_lib.query_windows(
                    cid, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), nchunks, chunk_len, D, 64, 7, 0, mn.data_ptr(), mx.data_ptr(), sm.data_ptr(),
                    None, stream())), args.steps)
                del mn, mx, sm
            if "dl" in only:
                rec["dl_decompress_torch_a_gt_b_ms"] = median_ms(torch_l, args.steps)
            if "dc" in only:
                rec["dc_decompress_torch_change_ms"] = median_ms(torch_c, args.steps)
            if "l_filter_linear_a_gt_b_ms" in rec and "f_filter_rows_band_ms" in rec:
                rec["l_over_f"] = round(rec["l_filter_linear_a_gt_b_ms"] / rec["f_filter_rows_band_ms"], 3)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    measure(codec, x, "walk")
    if "const" in only:
        view = torch.int16 if esz == 2 else torch.int8
        const = torch.full((nchunks * chunk_len,), 0x1234 if esz == 2 else 0xA5, dtype=torch.int32, device=dev).to(view).view(x.dtype)
        del x
        measure("delta", const, "constant")
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(head) + "\n")
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
    if not all(r["ok"] for r in lines):
        sys.exit("filter_linear differs from decompress + torch")


if __name__ == "__main__":
    main()
