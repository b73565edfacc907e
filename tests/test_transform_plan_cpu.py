"""CPU tests of the stand-alone transforms' decode plan (sprintz_amd/csrc/transform_plan.h): which form decodes a stream, cut into which
pieces, with which runs and levels, and where every array lies in d_tmp is plain integer arithmetic on the shape, the pointers' low bits and
SPRINTZ_MI355X_TRANSFORM_CHAIN -- and sprintz_mi355x_transform_tmp_bytes is derived from the same description.  tests/transform_plan_probe.cpp
includes the header, is built with g++ -- which is itself the check that it holds no HIP -- and answers one query per line.

1. the sweep: esz 1 / 2, delta / double delta, every ndims in 1 .. 1 100 plus 2 047 and 65 535, rows in {1, 2, 5, 16, 17, 64, 65, 200, 256,
   257, 1 000, 4 097, 16 384, 16 385, 70 001}, 0 / 1 / 3 extra elements, source and destination low bits in {0, 1 (uint8 only), 2, 4, 8},
   the setting default / "0" / "1".  For every case: every array inside [0, tmp_bytes) and no two overlapping (all of a call's arrays are
   live together), exactly one form with only that form's parts, the same answer twice.  And the size is capped, so that it is not "twice the
   stream": tmp_bytes <= 1.25 x stream bytes + 64 KiB;
2. the defect this tier was written for, pinned on five named shapes;
3. the GPU table (tests/transform_drive.py) replayed: every row's branch label against the plan, with 256 CUs."""
import shutil
import subprocess

import pytest

from transform_drive import KINDS, OVERRUN, TABLE, build_probe, length, matches, query

CUS = 256


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    return build_probe(tmp_path_factory.mktemp("transform_plan"))


@pytest.fixture(scope="module")
def sweep(probe):
    out = subprocess.run([probe.exe], input="sweep\n", capture_output=True, text=True, check=True).stdout.splitlines()
    return out[:-1], out[-1]


CAP = "tmp_bytes above 1.25 x stream"


def test_properties_over_the_sweep(sweep):
    violations, last = sweep
    shapes, cases = int(last.split("shapes=")[1].split()[0]), int(last.split("cases=")[1].split()[0])
    assert shapes == 2 * 2 * 1102 * 15 * 3
    assert cases == 2 * 1102 * 15 * 3 * 3 * (5 * 5 + 4 * 4)
    violations = [v for v in violations if CAP not in v]
    assert not violations, (len(violations), violations[:10])


def test_the_size_is_capped_over_the_sweep(sweep):
    """tmp_bytes <= 1.25 x stream bytes + 64 KiB: the size is not "twice the stream".  (What broke it first were 65 535 columns in 2 or 3
    rows: the generic levels placed their top level -- a single run whose summary nothing reads -- as two or four arrays of one row each,
    524 288 bytes for a stream of 131 076.  The top level has no arrays any more and is not reduced into.)  The peak over the streams of
    more than 1 MiB is 1.07 x: one load a run, 64 pieces a row, double delta."""
    violations, last = sweep
    over = [v for v in violations if CAP in v]
    assert not over, (len(over), over[:12])
    assert float(last.split("worst_ratio_above_1MiB=")[1]) <= 1.25


# (tag, kind) -> (bytes the launcher took from d_tmp, bytes sprintz_mi355x_transform_tmp_bytes reported) before the size was derived from the plan
PINNED = {
    ("overrun-u16x376-9rows", "doubledelta"): (12_288, 12_174),
    ("overrun-u16x496-29rows", "delta"): (17_920, 17_868),
    ("overrun-u8x140-77rows", "doubledelta"): (13_312, 13_187),
    ("overrun-u8x63-212rows+1", "doubledelta"): (13_824, 13_765),
    ("overrun-u16x512-16384rows", "doubledelta"): (17_895_424, 6_582_336),
}


@pytest.mark.parametrize("tag,kind", list(PINNED), ids=[f"{t}-{k}" for t, k in PINNED])
def test_the_scratch_covers_what_the_wave_scan_takes(probe, tag, kind):
    """The size counted one summary per 16 rows; the wave scan places one per RUN, and with one load a run and 22 .. 64 pieces a row a run is
    4 .. 8 rows.  Taken from d_tmp (level 1 + the levels above it) against what was reported:
        uint16 x 376, 9 rows, double delta            12 288 against     12 174   (3 runs)
        uint16 x 496, 29 rows, delta                  17 920 against     17 868
        uint8 x 140, 77 rows, double delta            13 312 against     13 187   (4-byte pieces, 35 a row)
        uint8 x 63, 212 rows + 1, double delta        13 824 against     13 765   (1-byte pieces, 63 a row)
        uint16 x 512, 16 384 rows, double delta   17 895 424 against  6 582 336   (4 096 runs of one load: 11.3 MB past the end)
    The probe restates both sides of that (`parent_used`, `parent`).  Today's plan takes the same bytes less the generic levels' top level,
    which was placed but read by nothing (in the first three shapes the excess lay inside it); no shape changed its form or its runs, and the
    size is what the plan takes, rounded to 64 bytes, + 64."""
    row, = [r for r in OVERRUN if r.tag == tag]
    took, reported = PINNED[tag, kind]
    n = length(row, probe, CUS)
    for chain in (-1, 0):
        got, = probe(query(row, kind, n, chain, CUS))
        assert got["family"] == "tr_wave" and int(got["parent_used"]) == took and int(got["parent"]) == reported and took > reported, got
        ends = [int(a.split(":")[1]) + int(a.split(":")[2]) for a in got["arrays"].split(",")]
        used = int(got["used"])
        assert max(ends) == used and took - 4 * 1024 <= used <= took, got
        assert used <= int(got["tmp_bytes"]) <= used + 128, got


@pytest.mark.parametrize("row", TABLE, ids=[r.tag for r in TABLE])
def test_the_gpu_table_replayed(probe, row):
    n = length(row, probe, CUS)
    for kind in KINDS:
        got, = probe(query(row, kind, n, -1, CUS))
        assert not matches(row.branch, got, CUS), (row.tag, kind, "default", matches(row.branch, got, CUS), got)
        zero, = probe(query(row, kind, n, 0, CUS))
        want0 = row.branch0 if row.branch0 is not None else row.branch
        assert not matches(want0, zero, CUS), (row.tag, kind, "0", matches(want0, zero, CUS), zero)
        assert (row.branch0 is not None) == (got["family"] != zero["family"]), (row.tag, got["family"], zero["family"])
        assert int(got["used"]) <= int(got["tmp_bytes"]) and int(zero["used"]) <= int(zero["tmp_bytes"])
