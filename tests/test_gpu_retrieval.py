"""cuda_ba.retrieval_query (csrc/retrieval.hip) against the fp64 restatement
(tests/retrieval_ref.py): masked scores and top-k within the derived bound of
an fp32 dot product, planted matches, ties, the NaN mask, bit identity between
batched and single queries, refusals."""
import functools

import numpy as np
import pytest
import torch

import retrieval_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4), (63, 128), (64, 4096), (65, 4096), (257, 4096)]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64).cpu().numpy()


@functools.lru_cache(maxsize=None)
def rows_of(N, D):
    return R.unit_rows(N, D, seed=7 * N + D)


def on_device(db, pad):
    """the rows on the device with a leading dimension of D + pad; the padding holds NaN"""
    N, D = db.shape
    full = torch.full((N, D + pad), float("nan"), device="cuda")
    full[:, :D] = T(db)
    return full[:, :D]


@functools.lru_cache(maxsize=None)
def queries(N, Q):
    """unsorted, with a repeat (Q >= 3), always with the last and the first row"""
    rng = np.random.default_rng(100 * N + Q)
    q = rng.integers(0, N, Q)
    q[0] = N - 1
    if Q >= 3:
        q[1], q[2] = 0, N - 1
    if Q >= 9:
        q[5] = q[7] = N // 2
    return tuple(int(v) for v in q)


@functools.lru_cache(maxsize=None)
def reference(N, D, Q, skip):
    return R.scores(rows_of(N, D), queries(N, Q), skip)


@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("N,D", SHAPES)
def test_scores_and_topk_against_fp64(N, D, pad, poisoned):
    import cuda_ba
    db = on_device(rows_of(N, D), pad)
    assert db.stride(0) == D + pad
    for Q in (1, 3, 9):
        qr = queries(N, Q)
        for skip in (0, 1, 50):
            ref, bound = reference(N, D, Q, skip)
            for top_k in (1, 10, 32):
                val, idx, sc = cuda_ba.retrieval_query(db, qr, skip, top_k=top_k, return_scores=True)
                val, idx, sc = val.cpu().numpy(), idx.cpu().numpy(), sc.cpu().numpy()
                assert val.shape == (Q, top_k) and idx.shape == (Q, top_k) and sc.shape == (Q, N)
                tag = (N, D, pad, Q, skip, top_k)
                for q, n in enumerate(qr):
                    end = R.candidate_end(n, skip)
                    # every score: within its bound inside the candidate range, -inf outside
                    assert (np.abs(sc[q, :end] - ref[q, :end]) <= bound[q, :end]).all(), tag
                    assert np.isneginf(sc[q, end:]).all(), tag
                    cnt = min(top_k, end)
                    # the tail
                    assert np.isneginf(val[q, cnt:]).all() and (idx[q, cnt:] == -1).all(), tag
                    if cnt == 0:
                        continue
                    v, i = val[q, :cnt].astype(np.float64), idx[q, :cnt]
                    assert (i >= 0).all() and (i < end).all() and len(set(i.tolist())) == cnt, tag
                    assert (np.diff(v) <= 0).all(), tag
                    # each pick's own fp64 score
                    assert (np.abs(ref[q, i] - v) <= bound[q, i]).all(), tag
                    # order statistics are 1-Lipschitz in the max norm
                    want = np.sort(ref[q, :end])[::-1][:cnt]
                    assert (np.abs(v - want) <= bound[q, :end].max()).all(), tag
                    # and the selection is exact on the kernel's own scores: values bitwise, ties by row
                    ev, ei = R.topk(sc[q].astype(np.float64), top_k)
                    assert np.array_equal(ei, idx[q]) and np.array_equal(ev.astype(np.float32), val[q]), tag


def test_planted_matches_are_found(poisoned):
    """each query is a 0.2-noise copy of one earlier row: the top-1 row is exact"""
    import cuda_ba
    N0, Q, D, skip = 200, 9, 128, 50
    rng = np.random.default_rng(3)
    db = R.unit_rows(N0 + Q, D, seed=11).astype(np.float64)
    src = rng.permutation(N0 - skip)[:Q]
    for q in range(Q):
        noise = rng.normal(size=D)
        db[N0 + q] = db[src[q]] + 0.2 * noise / np.linalg.norm(noise)
    db = (db / np.linalg.norm(db, axis=1, keepdims=True)).astype(np.float32)
    qr = list(range(N0, N0 + Q))
    ref, bound = R.scores(db, qr, skip)
    top2 = np.sort(ref, axis=1)[:, -2:]
    assert (np.argmax(ref, axis=1) == src).all()
    assert (top2[:, 1] - top2[:, 0] > 2 * bound.max()).all()     # the planted gap exceeds twice the bound
    val, idx = cuda_ba.retrieval_query(T(db), qr, skip)
    assert idx.cpu().numpy()[:, 0].tolist() == src.tolist()
    assert (np.abs(val.cpu().numpy()[:, 0] - top2[:, 1]) <= bound.max()).all()


def test_equal_scores_come_by_ascending_row(poisoned):
    import cuda_ba
    N, D = 70, 128
    db = rows_of(N, D).copy()
    noise = R.unit_rows(1, D, seed=5)[0]
    twin = db[N - 1] + 0.1 * noise
    twin /= np.linalg.norm(twin)
    for r in (40, 5, 17):
        db[r] = twin                      # exact duplicates, far above every other score
    val, idx = cuda_ba.retrieval_query(T(db), [N - 1], 0, top_k=4)
    v = bits(val)[0]
    assert idx.cpu().numpy()[0, :3].tolist() == [5, 17, 40]
    assert v[0] == v[1] == v[2] != v[3]
    # a table of one repeated row: every score equal, the rows 0 .. top_k - 1
    same = np.tile(twin, (300, 1)).astype(np.float32)
    val, idx = cuda_ba.retrieval_query(T(same), [299, 280], 10, top_k=32)
    assert idx.cpu().numpy().tolist() == [list(range(32))] * 2
    assert len(set(bits(val).ravel().tolist())) == 1


@pytest.mark.parametrize("skip", [0, 50])
def test_rows_outside_the_candidate_range_reach_no_output(skip, poisoned):
    """rows at or beyond n - skip_window, other than the query rows, hold NaN"""
    import cuda_ba
    N, D = 257, 4096
    db = rows_of(N, D)
    clean = T(db)
    for qr in ([200], [130], [60, 200, 7], list(queries(N, 9))):
        end = max(R.candidate_end(n, skip) for n in qr)
        dirty = db.copy()
        dirty[end:] = np.nan
        for n in qr:
            dirty[n] = db[n]
        if end > 0:
            assert not np.isnan(dirty[:end]).any()
        a = cuda_ba.retrieval_query(clean, qr, skip, top_k=10, return_scores=True)
        b = cuda_ba.retrieval_query(T(dirty), qr, skip, top_k=10, return_scores=True)
        for x, y in zip(a, b):
            assert np.array_equal(bits(x), bits(y)), (skip, qr)


def test_bits_do_not_depend_on_the_batch_or_the_workspace(poisoned):
    import _dpvo_hot as H
    import cuda_ba
    N, D, skip, top_k = 257, 4096, 1, 10
    db = T(rows_of(N, D))
    qr = list(queries(N, 9))
    batched = [bits(x) for x in cuda_ba.retrieval_query(db, qr, skip, top_k=top_k, return_scores=True)]
    again = [bits(x) for x in cuda_ba.retrieval_query(db, qr, skip, top_k=top_k, return_scores=True)]
    H.set_poison(0x00)
    zeroed = [bits(x) for x in cuda_ba.retrieval_query(db, qr, skip, top_k=top_k, return_scores=True)]
    H.set_poison(0xFF)
    for a, b, c in zip(batched, again, zeroed):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    for q, n in enumerate(qr):          # one at a time, in a longer table, as part of another batch
        single = [bits(x) for x in cuda_ba.retrieval_query(db, [n], skip, top_k=top_k, return_scores=True)]
        for a, b in zip(batched, single):
            assert np.array_equal(a[q:q + 1], b), (q, n)
    shorter = [bits(x) for x in cuda_ba.retrieval_query(db[:201], [200, 7, 200], skip, top_k=top_k, return_scores=True)]
    longer = [bits(x) for x in cuda_ba.retrieval_query(db, [7, 200], skip, top_k=top_k, return_scores=True)]
    assert np.array_equal(shorter[0][0], longer[0][1]) and np.array_equal(shorter[1][0], longer[1][1])
    assert np.array_equal(shorter[0][1], longer[0][0]) and np.array_equal(shorter[0][2], shorter[0][0])
    assert np.array_equal(shorter[2][0], longer[2][1][:201])


def test_refusals(poisoned):
    import _dpvo_hot as H
    import cuda_ba
    db = T(rows_of(63, 128))
    with pytest.raises(RuntimeError, match="GPU"):
        cuda_ba.retrieval_query(db.cpu(), [3], 0)
    with pytest.raises(RuntimeError, match="float32"):
        cuda_ba.retrieval_query(db.half(), [3], 0)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        cuda_ba.retrieval_query(db[:, :126].contiguous(), [3], 0)
    with pytest.raises(RuntimeError, match="ld"):
        cuda_ba.retrieval_query(db[:, :126].contiguous()[:, :124], [3], 0)          # ld = 126
    with pytest.raises(RuntimeError, match="ld"):
        cuda_ba.retrieval_query(db.view(-1).as_strided((63, 128), (64, 1)), [3], 0)  # ld < D
    for top_k in (0, 33, -1):
        with pytest.raises(RuntimeError, match="top_k"):
            cuda_ba.retrieval_query(db, [3], 0, top_k=top_k)
    for row in (-1, 63):
        with pytest.raises(RuntimeError, match="outside"):
            cuda_ba.retrieval_query(db, [3, row], 0)
        with pytest.raises(RuntimeError, match="outside"):
            cuda_ba.retrieval_query(db, torch.tensor([row], device="cuda"), 0)
    with pytest.raises(RuntimeError, match="skip_window"):
        cuda_ba.retrieval_query(db, [3], -1)
    # a workspace one byte short, straight through the C ABI
    lib = H.lib()
    need = lib.dpvo_retrieval_workspace_bytes(2, 63, 1)
    qr = torch.tensor([5, 9], device="cuda")
    val, idx = torch.zeros(2, 1, device="cuda"), torch.zeros(2, 1, dtype=torch.long, device="cuda")
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    args = (H.ptr(db), 128, 63, 128, H.ptr(qr), 2, 0, 1, H.ptr(val), H.ptr(idx), H.ptr(None), H.ptr(ws))
    assert lib.dpvo_retrieval_query(*args, need - 1, H.stream_of(db)) != 0
    assert b"workspace" in lib.dpvo_hot_last_error()
    assert lib.dpvo_retrieval_query(*args, need, H.stream_of(db)) == 0
    assert idx.cpu().numpy().ravel().tolist() == R.topk(R.scores(rows_of(63, 128), [5], 0)[0][0], 1)[1].tolist() + \
        R.topk(R.scores(rows_of(63, 128), [9], 0)[0][0], 1)[1].tolist()
    # no queries: empty outputs, no launch
    val, idx = cuda_ba.retrieval_query(db, [], 0, top_k=3)
    assert val.shape == (0, 3) and idx.shape == (0, 3)
