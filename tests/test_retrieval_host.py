"""Loop-closure retrieval, host side (no GPU): the restatement's state machine
against the recorded run of the reference's RetrievalNetVLAD, DPVO's refusal
with half of the loop closer's arguments, and the C-ABI bindings."""
import ctypes
from types import SimpleNamespace

import pytest

import retrieval_ref as R


def test_restatement_replays_the_reference_recording():
    """every detect_loop return and the found / prev_loop_closes lists after
    it, event for event; the script detects the planted revisit twice"""
    fx = R.load_fixture()
    d = R.Detector(int(fx["skip_window"]), int(fx["nms"]))
    desc = fx["desc"]
    assert R.replay(fx, d, lambda n, t: d.insert(n, desc[t])) == 2
    assert (fx["events"][:, 0] == R.OP_KEYFRAME).sum() >= 3


def test_recorded_decisions_are_far_from_the_threshold():
    """no top-1 score of the script lies within 0.05 of LOOP_RETR_THRESH = 0.5,
    so fp32 and fp64 scores take the same decisions"""
    assert R.top1_margin(R.load_fixture()) > 0.05


@pytest.mark.parametrize("kwargs", [dict(nvlad_db=object()), dict(loop_frontend=object()), dict()])
def test_loop_enabled_needs_both_arguments(kwargs):
    from dpvo.dpvo import DPVO
    with pytest.raises(NotImplementedError, match="loop.*nvlad_db.*loop_frontend"):
        DPVO(SimpleNamespace(loop_enabled=True), None, **kwargs)


def test_frontend_contract_is_checked():
    from dpvo.loop_closure import LongTermLoopClosure
    with pytest.raises(TypeError, match="tracks"):
        LongTermLoopClosure(None, None, None, SimpleNamespace(match=lambda a, b: None), 4, 4)


def test_ctypes_signatures_of_the_retrieval_symbols():
    import _dpvo_hot as H
    p, i64, i, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
    assert H._SIGNATURES["dpvo_retrieval_workspace_bytes"] == (sz, [i64, i64, i])
    assert H._SIGNATURES["dpvo_retrieval_query"] == (i, [p, i64, i64, i, p, i64, i64, i, p, p, p, p, sz, p])
    lib = H.lib()
    assert lib.dpvo_retrieval_workspace_bytes(3, 100, 1) >= 3 * 100 * 4
    assert lib.dpvo_retrieval_workspace_bytes(3, 100, 0) == 0 and lib.dpvo_retrieval_workspace_bytes(3, 100, 33) == 0
    # the entry point checks its arguments before it touches the device
    for bad in [dict(D=6), dict(ld=60), dict(ld=66), dict(top_k=0), dict(top_k=33), dict(ws=0)]:
        a = dict(D=64, ld=64, top_k=1, ws=4096)
        a.update(bad)
        rc = lib.dpvo_retrieval_query(p(256), a["ld"], 10, a["D"], p(256), 1, 0, a["top_k"], p(256), p(256), p(0),
                                      p(256), a["ws"], p(0))
        assert rc != 0, bad
        assert b"dpvo_retrieval_query" in lib.dpvo_hot_last_error()


def test_shim_refuses_cpu_tensors():
    import torch
    import cuda_ba
    with pytest.raises(RuntimeError, match="GPU"):
        cuda_ba.retrieval_query(torch.zeros(4, 8), [3], 0)
