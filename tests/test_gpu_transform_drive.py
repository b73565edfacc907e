"""GPU tests (-m gpu): the stand-alone transforms' scan decoders (csrc/transforms.hip) driven through every boundary their state crosses, at
the smallest stream that reaches it -- tests/transform_drive.py is the table, the inputs and the numpy reference; tests/test_transform_plan_cpu.py
confirms on the CPU that every row sits on the branch it names.

Every case calls sprintz_mi355x_transform_decode_device itself: source and destination are views into larger tensors at the row's byte
offsets, 256 guard bytes on both sides of the destination; d_tmp is exactly sprintz_mi355x_transform_tmp_bytes bytes filled with 0xA5, with a
guard of 2 x stream + 64 KiB behind it in the same tensor (large enough for anything a mis-sized scratch could take, so that an overrun fails
an assertion, not the device); the decode runs twice into the same scratch, not cleared in between, the second time under the other form where
the shape has two (SPRINTZ_MI355X_TRANSFORM_CHAIN default against "0"); and the dispatch counters say which form ran, both times.
The expected output never comes from a GPU encode."""
import ctypes as C

import numpy as np
import pytest

from dispatch import ran
from transform_drive import FILL_DEST, FILL_TMP, GUARD, KINDS, TABLE, build_probe, inputs, length, matches, query, units

pytestmark = pytest.mark.gpu

ORACLE_MAX_BYTES = 4 << 20


@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import sprintz_amd  # noqa: F401
    return build_probe(tmp_path_factory.mktemp("transform_drive")), torch.cuda.get_device_properties(0).multi_processor_count


def first_wrong(got, want, D, where):
    i = int(np.flatnonzero(got != want)[0])
    r, c = divmod(i, D)
    at = f"; that column's impulse is in row {where[c]}" if where and c in where else ""
    return f"first wrong sample in row {r}, column {c}: {int(got[i])} where {int(want[i])} is due{at}"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("row", TABLE, ids=[r.tag for r in TABLE])
def test_drive(gpu, oracle, monkeypatch, row, kind):
    import torch
    from sprintz_amd import _lib
    probe, cus = gpu
    esz, D = row.esz, row.D
    n = length(row, probe, cus)
    nbytes = n * esz
    plans = probe(query(row, kind, n, -1, cus), query(row, kind, n, 0, cus))
    # the row is on its branch on THIS device (the CPU tier says so for 256 CUs)
    assert not matches(row.branch, plans[0], cus), (row.tag, matches(row.branch, plans[0], cus))
    two_forms = plans[0]["family"] != plans[1]["family"]
    assert two_forms == (row.branch0 is not None)
    unit_rows = sorted(set(units(plans[0])) | set(units(plans[1])))
    k = _lib.TRANSFORM_DELTA if kind == "delta" else _lib.TRANSFORM_DOUBLEDELTA
    tmp_bytes = int(_lib.transform_tmp_bytes(k, esz, n, D))
    assert tmp_bytes == int(plans[0]["tmp_bytes"]), "the library and the probe size the scratch from one description"

    sbuf = torch.zeros(GUARD + 16 + nbytes, dtype=torch.uint8, device="cuda")
    dbuf = torch.empty(2 * GUARD + 16 + nbytes, dtype=torch.uint8, device="cuda")
    tbuf = torch.empty(tmp_bytes + 2 * nbytes + (64 << 10), dtype=torch.uint8, device="cuda")
    assert sbuf.data_ptr() % 256 == 0 and dbuf.data_ptr() % 256 == 0 and tbuf.data_ptr() % 256 == 0
    s0, d0 = GUARD + row.src_off, GUARD + row.dst_off
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    tbuf.fill_(FILL_TMP)
    for name, y, x, where in inputs(row, kind, n, unit_rows, seed=len(row.tag) * 131 + n % 1009):
        what = f"{row.tag} ({row.why}), {kind}, input {name}, unit boundaries every {unit_rows} rows"
        if name == "random" and nbytes <= ORACLE_MAX_BYTES:
            cont, _ = oracle.transform_encode(KINDS.index(kind), x, D)
            assert np.array_equal(cont[6:].view(y.dtype)[:n], y), what
        sbuf[s0:s0 + nbytes] = torch.from_numpy(y.view(np.uint8))
        for call in (0, 1):
            setting = "0" if (call == 1 and two_forms) else None
            if setting is None:
                monkeypatch.delenv("SPRINTZ_MI355X_TRANSFORM_CHAIN", raising=False)
            else:
                monkeypatch.setenv("SPRINTZ_MI355X_TRANSFORM_CHAIN", setting)
            family = plans[1 if setting == "0" else 0]["family"]
            dbuf.fill_(FILL_DEST)
            with ran(only=[family], **{family: 1}):
                _lib.check(_lib.transform_decode_device(k, esz, C.c_void_p(sbuf.data_ptr() + s0), n, D, C.c_void_p(dbuf.data_ptr() + d0),
                                                        C.c_void_p(tbuf.data_ptr()), stream))
            torch.cuda.synchronize()
            # the scratch guard first: an overrun is the finding, whatever it did to the samples
            over = torch.nonzero(tbuf[tmp_bytes:] != FILL_TMP)
            assert over.numel() == 0, f"{what}, call {call} ({family}): wrote {int(over.max()) + 1} bytes past the {tmp_bytes} of transform_tmp_bytes"
            out = dbuf.cpu().numpy()
            assert (out[:d0] == FILL_DEST).all() and (out[d0 + nbytes:] == FILL_DEST).all(), f"{what}, call {call} ({family}): guard bytes around the output touched"
            got = out[d0:d0 + nbytes].copy().view(x.dtype)
            assert np.array_equal(got, x), f"{what}, call {call} ({family}): " + first_wrong(got, x, D, where)
