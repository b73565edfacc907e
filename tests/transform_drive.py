"""The table that drives the stand-alone transforms' scan decoders (sprintz_amd/csrc/transforms.hip) through the boundaries their state
crosses, with the inputs and the reference of tests/test_gpu_transform_drive.py.  tests/test_transform_plan_cpu.py replays the same table
through the decode's plan on the CPU (sprintz_amd/csrc/transform_plan.h, tests/transform_plan_probe.cpp): every row names the branch it is
there for, and a row that drifts off its branch fails there, without a device.

These are not workload sizes: each row is the SMALLEST stream that reaches its branch.

A row's length is `rows` whole rows + `extra` elements (a ragged last row counts as a row of the scan), or -- the one-pass decode's rows --
a number of TILES + 5 rows, the tile's size asked of the probe, never written down here.  `branch` is what the plan must answer for the row
under the default SPRINTZ_MI355X_TRANSFORM_CHAIN; `branch0`, where the shape has two forms, what it must answer under "0"."""
import os
import shutil
import subprocess
from typing import NamedTuple, Optional

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = ("delta", "doubledelta")
DTYPES = {1: np.uint8, 2: np.uint16}
GUARD = 256                      # bytes on both sides of the destination
FILL_DEST, FILL_TMP = 0xC3, 0xA5


class Row(NamedTuple):
    tag: str
    esz: int
    D: int
    rows: object                 # whole rows, or ("tiles", n | "cus+3")
    extra: int
    branch: dict
    why: str
    branch0: Optional[dict] = None
    src_off: int = 0
    dst_off: int = 0


def wave(piece, loads, top, **more):
    return dict(family="tr_wave", piece=piece, run_loads=loads, top=top, **more)


LEVELS = dict(family="tr_levels", piece=0)
CHAIN = dict(family="tr_chain", piece=16)

TABLE = []

# ---- 1. the shapes whose level 1 (one summary per RUN of 4 .. 8 rows) overran a scratch sized for one summary per 16 rows
TABLE += [
    Row("overrun-u16x376-9rows", 2, 376, 9, 0, wave(16, 1, "levels", dv=47, run_rows=4, nruns=3), "3 runs of one load, 47 pieces a row: the smallest overrun (114 bytes, double delta)"),
    Row("overrun-u16x496-29rows", 2, 496, 29, 0, wave(16, 1, "levels", dv=62, run_rows=4, nruns=8), "62 pieces a row, delta overruns by 52 bytes"),
    Row("overrun-u8x140-77rows", 1, 140, 77, 0, wave(4, 1, "levels", dv=35, run_rows=4, nruns=20), "4-byte pieces, 35 a row"),
    Row("overrun-u8x63-212rows+1", 1, 63, 212, 1, wave(1, 1, "runs", dv=63, run_rows=4, nruns=54), "1-byte pieces, 63 a row, the one-workgroup scan above"),
    Row("overrun-u16x512-16384rows", 2, 512, 16384, 0, wave(16, 1, "levels", dv=64, run_rows=4, nruns=4096), "n16 = 256: the last stream of one load a run -- 4 096 runs of 4 rows, 11.3 MB past the old size"),
    Row("u16x512-16385rows", 2, 512, 16385, 0, wave(16, 4, "levels", dv=64, run_rows=16, nruns=1025), "n16 = 257: the first stream of 4 loads a run, where a run is 16 rows"),
]
# ---- 2. the run-length thresholds (n16 = 256 / 257, 1 024 / 1 025) and the 4 096-run switch, on 1-byte pieces where they are cheapest
for rows0, br, why in [
    (16384, wave(1, 1, "runs", nruns=4096, G=16), "n16 = 256: one load a run; scan_runs_kernel at D = 64 -- 16 groups of 256 runs"),
    (16385, wave(1, 4, "runs", nruns=1025, G=16), "n16 = 257: 4 loads a run"),
    (65536, wave(1, 4, "runs", nruns=4096, G=16), "n16 = 1 024: the last stream of 4 loads a run"),
    (65537, wave(1, 16, "runs", nruns=1025, G=16), "n16 = 1 025: 16 loads a run on 1-byte pieces"),
    (262144, wave(1, 16, "runs", nruns=4096, G=16), "the last 4 096-run stream on the one-workgroup scan"),
    (262145, wave(1, 16, "levels", nruns=4097), "4 097 runs, D <= 64: the generic levels above a wave-scan base of narrow rows"),
]:
    TABLE.append(Row(f"u8x64-ragged-{rows0}rows", 1, 64, rows0 - 1, 1, dict(br, dv=64), why))
TABLE += [
    # 16-byte pieces through the LDS hand-over (1 and 2 pieces a row)
    Row("u8x16-2^20rows", 1, 16, 1 << 20, 0, wave(16, 1, "runs", dv=1, nruns=4096), "n16 = 256 at one piece a row, LDS hand-over"),
    Row("u8x16-2^20+1rows", 1, 16, (1 << 20) + 1, 0, wave(16, 4, "runs", dv=1, nruns=1025), "n16 = 257 at one piece a row"),
    Row("u8x32-2^19rows", 1, 32, 1 << 19, 0, wave(16, 1, "runs", dv=2, nruns=4096), "n16 = 256 at two pieces a row, LDS hand-over"),
    Row("u8x32-2^19+1rows", 1, 32, (1 << 19) + 1, 0, wave(16, 4, "runs", dv=2, nruns=1025), "n16 = 257 at two pieces a row"),
    # (at two pieces a row 2^20 rows are n16 = 512 / 513: both sides take 4 loads -- the middle of the range, 2 048 / 2 049 runs)
    Row("u8x32-2^20rows", 1, 32, 1 << 20, 0, wave(16, 4, "runs", dv=2, nruns=2048), "4 loads a run, two pieces a row, 2 048 runs in 32 groups of 64"),
    Row("u8x32-2^20+1rows", 1, 32, (1 << 20) + 1, 0, wave(16, 4, "runs", dv=2, nruns=2049), "2 049 runs: the last group of scan_runs_kernel is short"),
    Row("u8x256-65536rows+4", 1, 256, 65536, 4, wave(4, 16, "levels", dv=64, nruns=1025), "n16 = 1 025: 16 loads a run on 4-byte pieces"),
]
# ---- 3. D on both sides of 64 at a few runs
TABLE += [
    Row("u8x64-200rows", 1, 64, 200, 0, wave(16, 1, "runs", dv=4, nruns=4, G=4), "D = 64: the one-workgroup scan, as many groups as runs"),
    Row("u8x68-200rows", 1, 68, 200, 0, wave(4, 1, "levels", dv=17, nruns=17), "D = 68: the generic levels above the base, 3 rows a load"),
]
# ---- 4. piece counts with idle lanes, and one row a load; the ragged stream drops to 1-byte pieces or, past 64 of them, to the levels
for dv in (3, 5, 9, 21, 22, 33, 63, 64):
    TABLE.append(Row(f"u8x{16 * dv}-70rows", 1, 16 * dv, 70, 0, wave(16, 1, "none" if 4 * (64 // dv) >= 70 else "runs" if 16 * dv <= 64 else "levels", dv=dv, run_rows=4 * (64 // dv)),
                     f"{dv} pieces a row: {64 // dv} rows a load, {64 - 64 // dv * dv} lanes idle"))
    TABLE.append(Row(f"u8x{16 * dv}-70rows+3", 1, 16 * dv, 70, 3, wave(1, 1, "runs", dv=48) if dv == 3 else LEVELS,
                     "ragged: 48 one-byte pieces a row" if dv == 3 else "ragged: more than 64 one-byte pieces a row, the generic levels alone"))
# ---- 5. the one-pass chained scan over more than one tile, and the two-pass form of the same stream
for D in (8, 16, 24, 32, 40, 48, 56, 64):
    TABLE.append(Row(f"chain-u16x{D}-3tiles", 2, D, ("tiles", 3), 0, dict(CHAIN, dv=D // 8, ntiles=4), f"{D // 8} pieces a row, {64 % (D // 8)} lanes idle in every load: 3 tiles + 5 rows",
                     branch0=dict(family="tr_wave", piece=16, dv=D // 8)))
for D in (1, 2, 4):
    TABLE.append(Row(f"chain-u16x{D}-3tiles", 2, D, ("tiles", 3), 0, dict(CHAIN, dv=1, M=8 // D, ntiles=4), f"{8 // D} rows inside a piece: 3 tiles + 5 pieces",
                     branch0=dict(family="tr_wave", piece=16, dv=1, M=8 // D)))
TABLE.append(Row("chain-u16x56-cus+3tiles", 2, 56, ("tiles", "cus+3"), 0, dict(CHAIN, dv=7, wgs="cus"), "more tiles than workgroups: a second ticket, 63 of 64 lanes active",
                 branch0=dict(family="tr_wave", piece=16, dv=7)))
# ---- 6. the generic levels alone: one to four levels, and the single pseudo-run
for rows0, extra, n in [(1, 0, 0), (2, 0, 1), (16, 0, 1), (17, 0, 2), (256, 0, 2), (257, 0, 3), (4097, 0, 4), (257, 5, 3)]:
    TABLE.append(Row(f"levels-u8x67-{rows0}rows" + (f"+{extra}" if extra else ""), 1, 67, rows0, extra, dict(LEVELS, nlevels=n),
                     "a single row: the pseudo-run above it" if n == 0 else f"{n} level{'s' if n > 1 else ''} above the rows" + (", ragged last row" if extra else "")))
# ---- 7. pointers off 16 bytes: the piece falls 16 -> 4 -> 2 / 1 -> the levels
for so, do, br in [(0, 0, CHAIN), (4, 0, wave(4, 1, "runs", dv=4)), (0, 4, wave(4, 1, "runs", dv=4)), (8, 8, wave(4, 1, "runs", dv=4)), (2, 2, wave(2, 1, "runs", dv=8))]:
    TABLE.append(Row(f"align-u16x8-src{so}-dst{do}", 2, 8, 3000, 0, br, "uint16 x 8 leaves the chained scan as soon as either pointer is off 16", src_off=so, dst_off=do,
                     branch0=wave(16, 1, "runs", dv=1) if br is CHAIN else None))
for so, do, br in [(0, 0, wave(16, 1, "levels", dv=5)), (4, 0, wave(4, 1, "levels", dv=20)), (0, 4, wave(4, 1, "levels", dv=20)), (8, 8, wave(4, 1, "levels", dv=20)),
                   (2, 2, LEVELS), (1, 0, LEVELS), (0, 1, LEVELS)]:
    TABLE.append(Row(f"align-u8x80-src{so}-dst{do}", 1, 80, 3000, 0, br, "uint8 x 80: 5 pieces of 16, 20 of 4, then 80 of 1 -- more than 64: the levels", src_off=so, dst_off=do))

assert len({r.tag for r in TABLE}) == len(TABLE)
OVERRUN = [r for r in TABLE if r.tag.startswith("overrun-")]


# ---------------------------------------------------------------- the probe
def build_probe(workdir):
    """g++ tests/transform_plan_probe.cpp -> ask(kind=, esz=, len=, D=, ...) -> {field: text}"""
    exe = os.path.join(str(workdir), "transform_plan_probe")
    subprocess.check_call([shutil.which("g++") or "g++", "-std=c++17", "-O2", os.path.join(HERE, "transform_plan_probe.cpp"), "-o", exe])

    def ask(*queries):
        text = "".join("plan" + "".join(f" {k}={int(v)}" for k, v in q.items()) + "\n" for q in queries)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(queries), out
        return [dict(tok.split("=", 1) for tok in line.split(" ")) for line in out]
    ask.exe = exe
    return ask


def query(row, kind, n, chain, cus):
    return dict(kind=KINDS.index(kind), esz=row.esz, len=n, D=row.D, src_lo=row.src_off % 16, dst_lo=row.dst_off % 16, chain=chain, cus=cus)


def length(row, ask, cus):
    """elements of the row's stream"""
    if not isinstance(row.rows, tuple):
        return row.rows * row.D + row.extra
    ntiles = cus + 3 if row.rows[1] == "cus+3" else row.rows[1]
    piece_elems = 16 // row.esz
    tile_e = int(ask(dict(kind=0, esz=row.esz, len=1024 * 16 * row.D, D=row.D))[0]["tile_e"])       # pieces of 16 bytes a tile
    assert tile_e > 0, row
    plus = 5 * max(row.D, piece_elems)               # 5 rows, or -- rows inside a piece -- 5 pieces, so that the stream stays whole pieces
    return ntiles * tile_e * piece_elems + plus


def matches(row_branch, answer, cus):
    """the fields of a branch label that the probe's answer does not carry out"""
    return {k: (v, answer.get(k)) for k, v in row_branch.items() if str(cus if v == "cus" else v) != answer.get(k)}


def units(answer):
    """rows of every unit whose boundary the plan's state crosses: a lane's rows, a load, a run, a scan group, a tile and a wave's part of it,
    every level's span"""
    u = set()
    if answer["family"] == "tr_levels":
        u.add(16)
    else:
        M, dv = int(answer["M"]), int(answer["dv"])
        load = 64 // dv * 4 * M
        u |= {4 * M, load}
        if answer["family"] == "tr_chain":
            tile = int(answer["tile_e"]) // dv * M
            u |= {tile // 8, tile}
        else:
            run, nruns = int(answer["run_rows"]), int(answer["nruns"])
            u.add(run)
            if answer["top"] == "runs":
                G = int(answer["G"])
                u.add((nruns + G - 1) // G * run)
    u |= {int(lv.split(":")[1]) for lv in answer["levels"].split(",") if lv}
    return sorted(u)


def impulse_rows(unit_rows, rows0):
    """the last row before and the first row after the first and the last boundary of every unit"""
    pos = set()
    for u in unit_rows:
        for m in {u, (rows0 - 1) // u * u}:
            if 0 < m < rows0:
                pos |= {m - 1, m}
    return sorted(pos) or [0]


# ---------------------------------------------------------------- the reference: plain numpy in int64, by the definition
def encode_ref(x, D, kind, esz):
    """y[r] = x[r] - x[r-1], or - 2 x[r-1] + x[r-2], per column, masked to the width"""
    xi = x.astype(np.int64)
    y = xi.copy()
    y[D:] -= xi[:-D]
    if kind == "doubledelta":
        y[D:] -= xi[:-D]
        if xi.size > 2 * D:
            y[2 * D:] += xi[:-2 * D]
    y &= (1 << 8 * esz) - 1
    return y.astype(DTYPES[esz])


def running_sums(a, block=256):
    """per-column running sums down the rows of a (rows, D) int64 array.  (numpy's accumulate along axis 0 walks row by row; summing inside
    blocks of rows and adding every block the total of the blocks before it gives the same integers several times faster)"""
    rows, D = a.shape
    nb = (rows + block - 1) // block
    if nb * block != rows:
        a = np.concatenate([a, np.zeros((nb * block - rows, D), np.int64)])
    c = np.cumsum(a.reshape(nb, block, D), axis=1)
    c[1:] += np.cumsum(c[:, -1, :], axis=0)[:-1, None, :]
    return c.reshape(nb * block, D)[:rows]


def decode_ref(y, D, kind, esz):
    """per-column cumulative sum of y (summed twice for double delta) in int64, masked"""
    n = y.size
    rows = (n + D - 1) // D
    yi = np.zeros(rows * D, np.int64)
    yi[:n] = y
    s = running_sums(yi.reshape(rows, D))
    if kind == "doubledelta":
        s = running_sums(s)
    s &= (1 << 8 * esz) - 1
    return s.astype(DTYPES[esz]).reshape(-1)[:n]


def inputs(row, kind, n, unit_rows, seed):
    """-> [(name, y, x, {column: impulse row} or None)]: (a) full-range random samples; (b) y all ones -- row counters / triangular numbers,
    wrapping at 256 / 65 536 rows; (c) y zero but for one impulse a column, in the last row before and the first after each unit boundary.
    x never comes from a device: (a) it is given, y follows by the definition and the sums of y must give x back; (b, c) it is written down in
    closed form -- r + 1 or (r + 1)(r + 2) / 2; 3 from the impulse's row on, or 3 (r - r0 + 1) -- and the sums of y must agree with it."""
    D, esz = row.D, row.esz
    rows0, mask, dt = (n + D - 1) // D, (1 << 8 * esz) - 1, DTYPES[esz]
    out = []
    x = np.random.default_rng(seed).integers(0, 1 << 8 * esz, n, dtype=dt)
    y = encode_ref(x, D, kind, esz)
    assert np.array_equal(decode_ref(y, D, kind, esz), x)
    out.append(("random", y, x, None))
    y = np.ones(n, dt)
    r = np.arange(rows0, dtype=np.int64) + 1
    x = np.repeat(((r if kind == "delta" else r * (r + 1) // 2) & mask).astype(dt), D)[:n]
    assert np.array_equal(decode_ref(y, D, kind, esz), x)
    out.append(("ones", y, x, None))
    pos = impulse_rows(unit_rows, rows0)
    r = np.arange(rows0, dtype=np.int64)[:, None]
    for v in range((len(pos) + D - 1) // D):
        r0 = np.full(D, rows0, np.int64)                       # (a column without an impulse: all zero)
        where = {c: p for c, p in enumerate(pos[v * D:(v + 1) * D]) if p * D + c < n}
        for c, p in where.items():
            r0[c] = p
        y = np.zeros(n, dt)
        y[[p * D + c for c, p in where.items()]] = 3
        ramp = np.maximum(r - r0[None, :] + 1, 0)
        x = ((3 * (ramp if kind == "doubledelta" else np.minimum(ramp, 1))) & mask).astype(dt).reshape(-1)[:n]
        assert np.array_equal(decode_ref(y, D, kind, esz), x)
        out.append((f"impulses-{v}", y, x, where))
    return out
