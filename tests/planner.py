"""The planner (sprintz_amd/csrc/plan.h) for the tests: tests/plan_probe.cpp, built with g++ once per process, and the questions put to it.

    ask("decode", q=QUERY["select"], esz=2, D=8, ...)   -> {"family": "dec_fast", "lds": 0, "grid": 64, ...}    every field but
                                                           `family` an int, the a/b/c groups (row, blkd, blke) strings
                                                        -> {"error": -2, "what": "..."} where the call fails
    ask_many([(op, fields), ...])                       -> one such dict per query, from ONE process

A field that is not named keeps plan.h's default -- the probe hard-wires none: a module that always plans one mode names its defaults in
plan_fixture(...).  QUERY holds the mode numbers of geom.h; tests/test_plan_cpu.py checks it against what the probe's `modes` prints."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

# geom.h: kQueryOff .. kQueryFloat
QUERY = {"off": 0, "materialize": 1, "reduce_only": 2, "window": 3, "gather": 4, "filter": 5, "select": 6, "aggregate": 7, "histogram": 8,
         "moments": 9, "groupby": 10, "extrema": 11, "linear": 12, "segment": 13, "float": 14}


CODEC = {"delta": 0, "xff": 1}


def bound(esz, chunk_len, D):
    """sprintz_mi355x_compress_bound: the slot stride ChunkedCodec uses"""
    hdr = (2 * D * (3 if esz == 1 else 4) + 7) // 8
    b = 8 + (chunk_len // (16 * D) + 1) * (hdr + 3) + chunk_len * esz + 32
    return (b + 127) & ~127


def plan_shape(codec, w, D, chunk_len, nchunks, lat=2048, blk_chunks=2049, mask=9, pair=1, no_fast=0, split=1):
    """the planner's inputs for a ChunkedCodec call under streams.options(...)"""
    esz = w // 8
    return dict(codec=CODEC[codec], esz=esz, D=D, chunk_len=chunk_len, nchunks=nchunks, total_len=nchunks * chunk_len, slot_stride=bound(esz, chunk_len, D),
                lat_chunks=lat, blk_chunks=blk_chunks, blk_kernels=mask, enc_pair=pair, no_fast=no_fast, split_lanes=split)


@functools.lru_cache(maxsize=None)
def probe_exe():
    """the built probe's path, or None without g++ (that this builds with g++ is the check that plan.h and geom.h hold no HIP)"""
    if not shutil.which("g++"):
        return None
    workdir = tempfile.mkdtemp(prefix="plan_probe_")
    atexit.register(shutil.rmtree, workdir, ignore_errors=True)
    exe = os.path.join(workdir, "plan_probe")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(HERE, "plan_probe.cpp"), "-o", exe])
    return exe


def run(text):
    """the probe's output lines for `text` on its stdin"""
    return subprocess.run([probe_exe()], input=text, capture_output=True, text=True, check=True).stdout.splitlines()


def parse(line):
    if line.startswith("error="):
        code, _, what = line[len("error="):].partition(" what=")
        return {"error": int(code), "what": what}
    got = dict(tok.split("=", 1) for tok in line.split(" "))
    return {k: v if k in ("family", "enc") or "/" in v else int(v) for k, v in got.items()}


def ask_many(queries):
    """queries: (op, {field: value}) -> one answer dict per query"""
    queries = list(queries)
    out = run("".join(op + "".join(f" {k}={int(v)}" for k, v in fields.items()) + "\n" for op, fields in queries))
    assert len(out) == len(queries), f"{len(queries)} queries, {len(out)} answers: {out[:5]}"
    return [parse(line) for line in out]


def ask(op, **fields):
    return ask_many([(op, fields)])[0]


def modes():
    """geom.h's kQuery* constants as the probe prints them: {"Off": 0, ...}"""
    line, = run("modes\n")
    return {k: int(v) for k, v in (tok.split("=") for tok in line.split())}


def available(required=False):
    """for a fixture's first line: skips without g++ (the CPU tier), or fails (required: the GPU tier's float rows, whose expected kernel is
    the planner's answer)"""
    if required:
        assert shutil.which("g++"), "the planner probe needs g++"
    elif probe_exe() is None:
        pytest.skip("no g++")


def family(got):
    """the family's name alone (the whole answer where the plan is an error), for the modules whose mode adds no field to the plan"""
    return got.get("family", got)


def split(got, fields=None):
    """-> (family, {every other field, or `fields` alone}), or the error's dict"""
    return got if "error" in got else (got["family"], {k: v for k, v in got.items() if k != "family" and (fields is None or k in fields)})


@pytest.fixture(scope="module")
def probe():
    """probe((op, fields), ...) -> one answer per query, from one process"""
    available()
    return lambda *queries: ask_many(queries)


def plan_fixture(required=False, shape=lambda got: got, **defaults):
    """a module's `plan` fixture: plan(**fields) -> shape(ask("decode", **defaults, **fields)), shape one of `family`, `split` or nothing"""
    @pytest.fixture(scope="module")
    def plan():
        available(required)
        return lambda **fields: shape(ask("decode", **dict(defaults, **fields)))
    return plan
