"""Host-side API checks (no GPU): tracker config presets and refusals, the
quaternion helper behind PatchGraph.init_from_prior, argument validation of
the native shims."""
import numpy as np
import pytest
import torch


def test_presets_match_reference_yaml_values():
    """dpvo_configs/*.yaml restated as data (values as in the reference files)."""
    from dpvo.config import make_cfg
    tum = make_cfg("tum_default")
    assert (tum.PATCHES_PER_FRAME, tum.REMOVAL_WINDOW, tum.OPTIMIZATION_WINDOW, tum.PATCH_LIFETIME) == (384, 22, 10, 13)
    assert tum.KEYFRAME_THRESH == 30.0 and tum.GRADIENT_BIAS is False and tum.MIXED_PRECISION is True
    c2 = make_cfg("default", PATCHES_PER_FRAME=96)
    assert c2.PATCHES_PER_FRAME == 96 and c2.KEYFRAME_THRESH == 15.0
    assert make_cfg("dpvo_2k").PATCHES_PER_FRAME == 192


def test_loop_closure_refused_not_ignored():
    """cfg.loop_enabled builds a loop closer in the reference (dpvo.py:101-102);
    here it is out of scope and must raise rather than be ignored."""
    from dpvo.config import make_cfg
    from dpvo.dpvo import DPVO
    with pytest.raises(NotImplementedError, match="loop"):
        DPVO(make_cfg("fast", loop_enabled=True), None, device="cpu")


def test_matrix_to_quaternion_matches_rotation_algebra():
    from scipy.spatial.transform import Rotation
    from dpvo.utils import matrix_to_quaternion
    r = Rotation.random(500, random_state=0)
    mats = r.as_matrix()
    # include the four branch regimes: near-identity and 180-degree turns about each axis
    extra = np.stack([np.eye(3), np.diag([1.0, -1.0, -1.0]), np.diag([-1.0, 1.0, -1.0]), np.diag([-1.0, -1.0, 1.0])])
    mats = np.concatenate([mats, extra])
    q = matrix_to_quaternion(torch.tensor(mats)).numpy()
    ref = Rotation.from_matrix(mats).as_quat()[:, [3, 0, 1, 2]]
    ref = np.where(ref[:, :1] < 0, -ref, ref)
    # 180-degree turns: w = 0 and the sign of the vector part is arbitrary
    same = np.minimum(np.abs(q - ref).max(1), np.abs(q + ref).max(1))
    assert same.max() < 1e-12
    assert np.all(q[:, 0] >= 0)
    with pytest.raises(ValueError):
        matrix_to_quaternion(torch.zeros(2, 3, 4))


def test_rowgemm_args_builder_fills_the_struct_fields():
    """update_ops._gemm_args on CPU tensors: every pointer, stride, K / N / M and
    the flags land in the RowGemmArgs field the C struct names; the row-tensor
    and M_dev checks carry the caller's name."""
    import update_ops as U
    K, M = 128, 5
    A = torch.zeros(9, K + 8, dtype=torch.float16)[:, :K]
    W, b = torch.zeros(K // 32, 384, 32, dtype=torch.float16), torch.zeros(384, dtype=torch.float16)
    idx, ridx = torch.arange(M), torch.arange(M)
    res32, out32 = torch.zeros(M, 388)[:, :384], torch.zeros(M, 392)[:, :384]
    res16, gate16 = torch.zeros(7, 384, dtype=torch.float16), torch.zeros(M, 384, dtype=torch.float16)
    out16 = torch.zeros(M, 396, dtype=torch.float16)[:, :384]
    ln = (torch.zeros(384), torch.ones(384), 1e-3)
    heads = (torch.zeros(4, 384, dtype=torch.float16), torch.zeros(4, dtype=torch.float16))
    ho = torch.zeros(M, 4, dtype=torch.float16)
    a = U._gemm_args("caller", W, K, b, A=A, a_idx=idx, M=M, flags=U.RES | U.WKB, res32=res32, res16=res16,
                     res16_idx=ridx, gate16=gate16, ln=ln, heads=heads, head_out=ho, out32=out32, out16=out16)
    want = dict(A=A.data_ptr(), lda=K + 8, a_idx=idx.data_ptr(), a_rows=9, W=W.data_ptr(), K=K, N=384, bias=b.data_ptr(),
                zero_row=U.zero_row(A.device, K).data_ptr(), M=M, res32=res32.data_ptr(), ldr=388,
                res16=res16.data_ptr(), res16_idx=ridx.data_ptr(), gate16=gate16.data_ptr(), ln_g=ln[0].data_ptr(),
                ln_b=ln[1].data_ptr(), head_w=heads[0].data_ptr(), head_b=heads[1].data_ptr(), head_out=ho.data_ptr(),
                out32=out32.data_ptr(), ldo32=392, out16=out16.data_ptr(), ldo16=396, flags=U.RES | U.WKB, M_dev=None)
    assert {k: getattr(a, k) for k in want} == want
    assert a.ln_eps == pytest.approx(1e-3)
    assert set(want) | {"ln_eps"} == {f[0] for f in U.RowGemmArgs._fields_}
    # a later GEMM of a chain: no A, no zero row, nothing of the epilogue
    g = U._gemm_args("caller", W, K, b)
    assert (g.A, g.zero_row, g.a_idx, g.res32, g.out16, g.ln_g, g.head_w, g.M_dev) == (None,) * 8
    assert (g.W, g.K, g.N, g.bias, g.M, g.flags, g.lda, g.ldr, g.ldo16) == (W.data_ptr(), K, 384, b.data_ptr(), 0, 0, 0, 0, 0)
    with pytest.raises(RuntimeError, match="caller: M_dev must be a device int64 scalar"):
        U._gemm_args("caller", W, K, b, M_dev=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="caller: res32 must be fp32"):
        U._gemm_args("caller", W, K, b, res32=res32.half())
    with pytest.raises(RuntimeError, match=r"caller: gate16 must be contiguous fp16"):
        U._gemm_args("caller", W, K, b, gate16=gate16[:, :380])


def test_group_by_key_bits_validated():
    import update_ops
    assert update_ops.key_bits_for(2048 * 192) == 19
    assert update_ops.key_bits_for(1) == 1
    with pytest.raises(RuntimeError, match="key_bits"):
        update_ops.group_by(torch.zeros(4, dtype=torch.int64), key_bits=65)
