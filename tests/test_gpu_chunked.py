"""Partition builds that take more than one key chunk (build_dev.hip's chunk
loop), every word against the oracle.

The workspace limit (LSMB_WORKSPACE_MB, read per build) bounds the regions +
counts of one chunk; at its 8 GiB default only the 1e9-key builds chunk.  At
16 MiB the 66-slice filter new(7 200 000, 0.01) takes 1 M keys in chunks of
(tests/golden/plan_table.json, partition_chunk_keys at 16 MiB):

    k  CUs  keys per chunk  chunks
    7  256         367 616       3
    7   64         593 536       2
    5  256         448 512       3
    5   64         830 976       2

so every case below runs at least two chunks: later chunks advance the key
pointer (fixed) or the absolute offsets (var-len), re-plan for their own size,
and accumulate onto the words the first (fresh) chunk wrote.
"""
import numpy as np
import pytest

import keygen
import lsmbloom

pytestmark = pytest.mark.gpu

N = 1_000_000
NB = 68_883_501
MAX_CHUNK = 830_976  # the largest chunk of the table above


@pytest.fixture(scope="module")
def ctx():
    c = lsmbloom.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def keys16():
    return keygen.key16(0xC4A2, 0, N)


@pytest.fixture(scope="module")
def ref16_k7(oracle, keys16):
    return oracle.build_fixed_mt(keys16, 16, NB, 7, 16)


@pytest.fixture
def small_workspace(monkeypatch):
    assert lsmbloom.params(7_200_000, 0.01) == (NB, 7)
    assert N > MAX_CHUNK
    monkeypatch.setenv("LSMB_WORKSPACE_MB", "16")


def _dev(a):
    import torch
    return torch.from_numpy(a).to(torch.device("cuda:0"))


def _garbage(seed):
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    w = torch.randint(-2**62, 2**62, (lsmbloom.num_words(NB),), generator=g, dtype=torch.int64)
    return w.to(torch.device("cuda:0"))


def _cmp(w, ref):
    import torch
    torch.cuda.synchronize()
    got = w.cpu().numpy().view(np.uint64)
    assert got.shape == ref.shape
    bad = np.nonzero(got != ref)[0]
    assert bad.size == 0, "first mismatching words: %s" % bad[:8]


def test_chunked_fixed16_fresh_k7(ctx, small_workspace, keys16, ref16_k7):
    # the LIST pass A on the first chunk only; later chunks accumulate
    assert lsmbloom.build_strategy(NB, N, 7) == "partition"
    w = _garbage(1)
    ctx.build_fixed_dev_new(_dev(keys16), 16, N, NB, 7, w)
    _cmp(w, ref16_k7)


def test_chunked_fixed16_accumulate(ctx, monkeypatch, keys16, ref16_k7):
    # 200 k keys at the default limit (one chunk), the rest at 16 MiB onto those words
    import torch
    first = 200_000
    assert lsmbloom.build_strategy(NB, first, 7) == "partition"
    assert lsmbloom.build_strategy(NB, N - first, 7) == "partition" and N - first > 593_536
    keys = _dev(keys16)
    w = torch.zeros(lsmbloom.num_words(NB), dtype=torch.int64, device=keys.device)
    ctx.build_fixed_dev(keys[:first], 16, first, NB, 7, w)
    monkeypatch.setenv("LSMB_WORKSPACE_MB", "16")
    ctx.build_fixed_dev(keys[first:], 16, N - first, NB, 7, w)
    _cmp(w, ref16_k7)


def test_chunked_fixed16_fresh_k5(ctx, oracle, small_workspace, keys16):
    # k != 7: the first chunk zeroes the words, then every chunk accumulates
    assert lsmbloom.build_strategy(NB, N, 5) == "partition"
    w = _garbage(3)
    ctx.build_fixed_dev_new(_dev(keys16), 16, N, NB, 5, w)
    _cmp(w, oracle.build_fixed_mt(keys16, 16, NB, 5, 16))


def test_chunked_fixed20_fresh_k7(ctx, oracle, small_workspace):
    # 20-B keys: pre-hashed into walk records, the record buffer sized by chunk
    data = keygen.stream_bytes(0xC4A3, N * 20)
    assert lsmbloom.build_strategy(NB, N, 7) == "partition"
    w = _garbage(4)
    ctx.build_fixed_dev_new(_dev(data), 20, N, NB, 7, w)
    _cmp(w, oracle.build_fixed_mt(data, 20, NB, 7, 16))


def test_chunked_varlen_fresh_k7(ctx, oracle, small_workspace):
    # var-len keys: offsets stay absolute into the data across chunks
    data, offs = keygen.varlen(N)
    assert lsmbloom.build_strategy(NB, N, 7) == "partition"
    w = _garbage(5)
    ctx.build_var_dev_new(_dev(data), _dev(offs.view(np.int64)), N, NB, 7, w)
    _cmp(w, oracle.build_var_mt(data, offs, NB, 7, 16))
