"""Restatement of the loop-closure retrieval in numpy fp64, for the tests:
the masked scores and their top-k (cuda_ba.retrieval_query), the derived
error bound of an fp32 dot product, and the loop-detection state machine
(dpvo.loop_closure.Retrieval) as a small class over host lists.
"""
import numpy as np


def unit_rows(n, d, seed):
    """n seeded unit-norm fp32 rows"""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def candidate_end(n, skip_window):
    return max(int(n) - int(skip_window), 0)


def scores(db, query_rows, skip_window):
    """-> (scores [Q, N] fp64 with -inf outside each query's candidate range,
    bound [Q, N]: the fp32 dot product's error bound 1.01 D 2^-24 sum |a_i b_i|,
    which holds for every summation order, FMA or not)"""
    db64 = np.asarray(db, np.float64)
    N, D = db64.shape
    q = db64[np.asarray(query_rows, np.int64)]
    s = q @ db64.T
    bound = 1.01 * D * 2.0 ** -24 * (np.abs(q) @ np.abs(db64).T)
    for k, n in enumerate(query_rows):
        s[k, candidate_end(n, skip_window):] = -np.inf
    return s, bound


def topk(score_row, top_k):
    """the top_k largest of one score row in non-increasing order, equal
    scores by ascending row, the tail (-inf, -1) -> (val [top_k], idx [top_k])"""
    order = np.lexsort((np.arange(score_row.size), -score_row))
    order = order[np.isfinite(score_row[order])][:top_k]
    val = np.full(top_k, -np.inf)
    idx = np.full(top_k, -1, np.int64)
    val[:order.size] = score_row[order]
    idx[:order.size] = order
    return val, idx


class Detector:
    """The loop-detection rules over a db the test holds on the host.

    insert(n, desc) / keyframe(k) / save_up_to(c) / detect_loop / confirm_loop
    with the meaning of dpvo.loop_closure.Retrieval; the search is scores() and
    topk() above in fp64."""

    def __init__(self, skip_window=50, nms=50):
        self.skip_window, self.nms = skip_window, nms
        self.pending = {}
        self.final = {}
        self.results = []
        self.found = []
        self.prev_loop_closes = []

    def insert(self, n, desc):
        self.pending[n] = np.asarray(desc, np.float64)

    def keyframe(self, k):
        old, self.pending = self.pending, {}
        for n, v in old.items():
            if n != k:
                self.pending[n - 1 if n > k else n] = v

    def save_up_to(self, c):
        for n in sorted(self.pending):
            if n > c:
                continue
            assert n not in self.final
            desc = self.final[n] = self.pending.pop(n)
            end = candidate_end(n, self.skip_window)
            if end == 0:
                self.results.append((n, 0.0, None))
                continue
            s = np.array([self.final[r] @ desc for r in range(end)])
            j = int(np.argmax(s))          # the first of equal maxima
            self.results.append((n, float(s[j]), j))

    def confirm_loop(self, i, j):
        assert i > j
        self.prev_loop_closes.append((i, j))

    def detect_loop(self, thresh, num_repeat=1):
        while self.results:
            i, score, j = self.results.pop(0)
            if score < thresh:
                continue
            assert i > j
            if any((i - a) ** 2 + (j - b) ** 2 < self.nms ** 2 for a, b in self.prev_loop_closes):
                continue
            self.found.append((i, j))
            if len(self.found) < num_repeat:
                continue
            latest = self.found[-num_repeat:]
            if 1 + i - latest[0][0] == num_repeat:
                a, b = latest[num_repeat // 2]
                return (a, max(b, 1))
        return None


# ---------------------------------------------------------------------------
# the recorded run of the reference's RetrievalNetVLAD (tests/golden/make_golden_retrieval.py)
# ---------------------------------------------------------------------------
OP_CALL, OP_KEYFRAME, OP_SAVE, OP_DETECT, OP_CONFIRM = range(5)


def load_fixture():
    import os
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "retrieval_ref.npz")))


def replay(fx, machine, call):
    """run the fixture's event script on `machine` (keyframe, save_up_to,
    detect_loop, confirm_loop, found, prev_loop_closes; call(n, t) inserts
    frame t as row n) and compare every detect_loop return and the two lists
    after it with the recording -> the number of detections"""
    thresh, repeat = float(fx["thresh"]), int(fx["repeat"])
    step = hits = 0
    last = None
    for op, a, b in fx["events"].tolist():
        if op == OP_CALL:
            call(a, b)
        elif op == OP_KEYFRAME:
            machine.keyframe(a)
        elif op == OP_SAVE:
            machine.save_up_to(a)
        elif op == OP_DETECT:
            last = machine.detect_loop(thresh, repeat)
            want = tuple(fx["returns"][step])
            assert (last if last is not None else (-1, -1)) == want, (step, last, want)
            if last is None:
                _compare_lists(fx, step, machine)
                step += 1
        elif op == OP_CONFIRM:   # always right after its detection
            assert last == (a, b)
            machine.confirm_loop(a, b)
            machine.found.clear()
            _compare_lists(fx, step, machine)
            step += 1
            hits += 1
    assert step == len(fx["returns"])
    return hits


def _compare_lists(fx, step, machine):
    for name, got in (("found", machine.found), ("prev", machine.prev_loop_closes)):
        lo, hi = fx[name + "_off"][step:step + 2]
        want = [tuple(p) for p in fx[name][lo:hi].tolist()]
        assert [tuple(int(v) for v in p) for p in got] == want, (name, step, got, want)


def top1_margin(fx):
    """the smallest |score - thresh| - bound over every top-1 score the script
    queries, in fp64 on the final rows: positive = no decision of the run
    depends on fp32 rounding"""
    d = Detector(int(fx["skip_window"]), int(fx["nms"]))
    desc = fx["desc"].astype(np.float64)
    worst = np.inf
    for op, a, b in fx["events"].tolist():
        if op == OP_CALL:
            d.insert(a, desc[b])
        elif op == OP_KEYFRAME:
            d.keyframe(a)
        elif op == OP_SAVE:
            d.save_up_to(a)
            for n, score, j in d.results:
                if j is not None:
                    bound = 1.01 * desc.shape[1] * 2.0 ** -24 * float(np.abs(d.final[n]) @ np.abs(d.final[j]))
                    worst = min(worst, abs(score - float(fx["thresh"])) - bound)
            d.results.clear()
    return worst
