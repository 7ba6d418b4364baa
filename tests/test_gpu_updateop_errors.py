"""Error outcomes of the update-operator entry points (csrc/updateop.hip,
groupby.hip, scatter.hip) straight through the C ABI: the return code and the
whole dpvo_hot_last_error() text of deliberately bad calls.  Every call fails
(or returns early) in the entry point's checks, ahead of its launches in the
source; the test asserts the outcomes, and that the operand buffer still holds
its zeros -- a smoke check, not proof that nothing ran.  The order
of an entry point's checks is part of its behaviour -- which message a call
with two faults gets, and which calls return 0 before a fault is looked at --
so cases with two faults pin it."""
import pytest
import torch

pytestmark = pytest.mark.gpu

P = "P"        # a valid device buffer (WS_BYTES long)
WS_BYTES = 1 << 16
E, D = 4, 2

# (entry point, arguments, return code, dpvo_hot_last_error() or None where the call succeeds)
CASES = [
    # dpvo_softagg_forward(dtype, f, ldf, s, lds, group, E, D, groups, eps, y, ws, ws_bytes, stream)
    ("dpvo_softagg_forward", (99, P, D, P, D, P, E, D, 2, 0.0, P, P, WS_BYTES, None), -1,
     "dpvo_softagg_forward: unsupported dtype"),
    ("dpvo_softagg_forward", (0, P, D, P, D, P, E, 3, 2, 0.0, P, P, WS_BYTES, None), -1,
     "dpvo_softagg_forward: feature dim must be even and positive"),
    ("dpvo_softagg_forward", (0, P, 1, P, D, P, E, D, 2, 0.0, P, P, WS_BYTES, None), -1,
     "dpvo_softagg_forward: row strides must be even and >= D"),
    ("dpvo_softagg_forward", (0, P, 1, P, D, P, -1, D, 2, 0.0, P, P, WS_BYTES, None), -1,      # sizes before strides
     "dpvo_softagg_forward: bad sizes"),
    ("dpvo_softagg_forward", (99, P, 1, P, D, P, E, D, 2, 0.0, P, P, WS_BYTES, None), -1,      # strides before dtype
     "dpvo_softagg_forward: row strides must be even and >= D"),
    ("dpvo_softagg_forward", (99, P, D, P, D, P, E, D, 0, 0.0, P, P, WS_BYTES, None), -1,      # dtype before groups == 0
     "dpvo_softagg_forward: unsupported dtype"),
    ("dpvo_softagg_forward", (0, P, D, P, D, P, 0, D, 0, 0.0, P, None, 0, None), 0, None),
    ("dpvo_softagg_forward", (0, P, D, P, D, P, 0, D, 2, 0.0, P, P, WS_BYTES, None), -1,
     "dpvo_softagg_forward: groups without edges"),
    ("dpvo_softagg_forward", (0, P, D, P, D, P, E, D, 2, 0.0, P, P, 16, None), -1,
     "dpvo_softagg_forward: workspace too small"),
    ("dpvo_softagg_forward", (0, P, D, P, D, P, E, D, 2, 0.0, P, None, WS_BYTES, None), -1,
     "dpvo_softagg_forward: workspace too small"),
    # dpvo_softagg_csr(dtype, f, ldf, s, lds, offs, perm, groups, max_groups, D, eps, y, stream)
    ("dpvo_softagg_csr", (0, P, D, P, D, P, P, P, 4, 3, 0.0, P, None), -1,
     "dpvo_softagg_csr: feature dim must be even and positive"),
    ("dpvo_softagg_csr", (0, P, D, P, 1, P, P, P, 4, D, 0.0, P, None), -1,
     "dpvo_softagg_csr: row strides must be even and >= D"),
    ("dpvo_softagg_csr", (0, P, D, P, D, None, P, P, 4, D, 0.0, P, None), -1, "dpvo_softagg_csr: CSR missing"),
    ("dpvo_softagg_csr", (0, P, D, P, D, P, P, None, 0, D, 0.0, P, None), -1,                 # CSR before max_groups
     "dpvo_softagg_csr: CSR missing"),
    ("dpvo_softagg_csr", (99, P, D, P, D, P, P, P, 4, D, 0.0, P, None), -1, "dpvo_softagg_csr: unsupported dtype"),
    ("dpvo_softagg_csr", (99, P, D, P, D, P, P, P, 0, D, 0.0, P, None), 0, None),             # max_groups before dtype
    # dpvo_softagg_csr_long(the same arguments)
    ("dpvo_softagg_csr_long", (0, P, D, P, D, P, P, P, 4, 0, 0.0, P, None), -1,
     "dpvo_softagg_csr_long: feature dim must be even and positive"),
    ("dpvo_softagg_csr_long", (0, P, 3, P, D, P, P, P, 4, D, 0.0, P, None), -1,
     "dpvo_softagg_csr_long: row strides must be even and >= D"),
    ("dpvo_softagg_csr_long", (0, P, D, P, D, P, None, P, 4, D, 0.0, P, None), -1, "dpvo_softagg_csr_long: CSR missing"),
    ("dpvo_softagg_csr_long", (2, P, D, P, D, P, P, P, 4, D, 0.0, P, None), -1,
     "dpvo_softagg_csr_long: dtype must be fp16 or fp32"),
    ("dpvo_softagg_csr_long", (99, P, D, P, D, P, P, P, 0, D, 0.0, P, None), -1,              # dtype before max_groups
     "dpvo_softagg_csr_long: dtype must be fp16 or fp32"),
    ("dpvo_softagg_csr_long", (1, P, D, P, D, P, P, P, 0, D, 0.0, P, None), 0, None),
    # dpvo_gather_rows(in_dtype, x, ldx, rows, idx, n, D, out_dtype, out, stream)
    ("dpvo_gather_rows", (0, P, D, E, P, E, 3, 0, P, None), -1,
     "dpvo_gather_rows: feature dim / row stride must be even"),
    ("dpvo_gather_rows", (0, P, 1, E, P, E, D, 0, P, None), -1,
     "dpvo_gather_rows: feature dim / row stride must be even"),
    ("dpvo_gather_rows", (0, P, D, E, P, -1, D, 0, P, None), -1, "dpvo_gather_rows: bad sizes"),
    ("dpvo_gather_rows", (99, P, D, E, P, E, D, 0, P, None), -1, "dpvo_gather_rows: unsupported dtype"),
    ("dpvo_gather_rows", (0, P, D, E, P, E, D, 99, P, None), -1, "dpvo_gather_rows: unsupported dtype"),
    ("dpvo_gather_rows", (99, P, D, E, P, 0, D, 99, P, None), 0, None),                       # n == 0 before the dtypes
    # dpvo_edge_targets(delta, ds, w, ws, centre, cs, cc, E, target, weight, stream)
    ("dpvo_edge_targets", (P, 4, P, 4, P, 2, 1, -1, P, P, None), -1, "dpvo_edge_targets: E >= 0 required"),
    ("dpvo_edge_targets", (P, 4, None, 4, P, 2, 1, E, P, P, None), -1, "dpvo_edge_targets: null operand"),
    ("dpvo_edge_targets", (None, 4, None, 4, None, 2, 1, 0, None, None, None), 0, None),
    # dpvo_group_by(key, n, key_bits, gid, offs, perm, groups, ws, ws_bytes, stream)
    ("dpvo_group_by", (P, -1, 8, P, P, P, P, P, WS_BYTES, None), -1, "dpvo_group_by: bad size"),
    ("dpvo_group_by", (P, E, 0, P, P, P, P, P, WS_BYTES, None), -1, "dpvo_group_by: key_bits must be 1..64"),
    ("dpvo_group_by", (P, E, 65, P, P, P, P, P, WS_BYTES, None), -1, "dpvo_group_by: key_bits must be 1..64"),
    ("dpvo_group_by", (P, E, 8, P, P, P, None, P, WS_BYTES, None), -1, "dpvo_group_by: groups output missing"),
    ("dpvo_group_by", (P, E, 8, P, P, P, P, P, 16, None), -1, "dpvo_group_by: workspace too small"),
    ("dpvo_group_by", (P, E, 40, P, P, P, P, None, WS_BYTES, None), -1, "dpvo_group_by: workspace too small"),
    # dpvo_window_keys(ii, jj, kk, E, M, base, ring, frames, key_kk, key_ij, ctx, jslot, flag, stream)
    ("dpvo_window_keys", (P, P, P, E, 0, 0, 8, 8, P, P, P, P, None, None), -1,
     "dpvo_window_keys: E >= 0, M > 0, ring > 0 and frames > 0 required"),
    ("dpvo_window_keys", (P, P, P, E, 4, 0, 8, 0, P, P, P, P, None, None), -1,
     "dpvo_window_keys: E >= 0, M > 0, ring > 0 and frames > 0 required"),
    ("dpvo_window_keys", (P, P, P, E, 4, 0, 8, 8, P, P, P, None, None, None), -1, "dpvo_window_keys: null operand"),
    ("dpvo_window_keys", (None, P, P, 0, 4, 0, 8, 8, P, P, P, None, None, None), 0, None),
    # dpvo_window_group_by(ii, jj, kk, E, M, base, ring, frames, kk_bits, ctx, jslot, flag, kk_gid, kk_offs, kk_perm,
    #                      kk_groups, ij_gid, ij_offs, ij_perm, ij_groups, jj_order, ws, ws_bytes, stream)
    ("dpvo_window_group_by", (P, P, P, -1, 4, 0, 8, 8, 8, P, P, None, P, P, P, P, P, P, P, P, None, P, WS_BYTES, None),
     -1, "dpvo_window_group_by: bad size"),
    ("dpvo_window_group_by", (P, P, P, E, 4, 0, 0, 8, 8, P, P, None, P, P, P, P, P, P, P, P, None, P, WS_BYTES, None),
     -1, "dpvo_window_group_by: M > 0, ring > 0 and frames > 0 required"),
    ("dpvo_window_group_by", (P, P, P, E, 4, 0, 8, 8, 23, P, P, None, P, P, P, P, P, P, P, P, None, P, WS_BYTES, None),
     -1, "dpvo_window_group_by: kk_bits must be 1..22"),
    ("dpvo_window_group_by", (P, P, P, E, 4, 0, 8, 8, 0, P, P, None, P, P, P, P, P, P, P, P, None, P, WS_BYTES, None),
     -1, "dpvo_window_group_by: kk_bits must be 1..22"),
    ("dpvo_window_group_by", (P, P, P, E, 4, 0, 8, 8, 8, P, P, None, P, P, P, P, P, None, P, P, None, P, WS_BYTES,
                              None), -1, "dpvo_window_group_by: CSR outputs missing"),
    ("dpvo_window_group_by", (P, P, P, E, 4, 0, 8, 8, 8, P, P, None, None, P, P, P, P, P, P, P, None, P, WS_BYTES,
                              None), -1, "dpvo_window_group_by: null operand"),
    ("dpvo_window_group_by", (P, P, P, E, 4, 0, 8, 8, 8, P, P, None, P, P, P, P, P, P, P, P, None, P, 16, None),
     -1, "dpvo_window_group_by: workspace too small"),
    # dpvo_neighbors_csr(jj, offs, perm, groups, max_groups, num_edges, ix, jx, stream)
    ("dpvo_neighbors_csr", (P, P, None, P, 4, E, P, P, None), -1, "dpvo_neighbors_csr: CSR missing"),
    ("dpvo_neighbors_csr", (P, P, P, P, 4, -1, P, P, None), -1, "dpvo_neighbors_csr: bad size"),
    ("dpvo_neighbors_csr", (P, P, P, P, 0, E, P, P, None), 0, None),
    # dpvo_append_edges(ii, jj, kk, E, ix, n, M, r, ii_out, jj_out, kk_out, stream)
    ("dpvo_append_edges", (P, P, P, E, P, 0, 4, 13, P, P, P, None), -1,
     "dpvo_append_edges: n >= 1, M >= 1, PATCH_LIFETIME >= 1 and E >= 0 required"),
    ("dpvo_append_edges", (P, P, P, -1, P, 2, 4, 13, P, P, P, None), -1,
     "dpvo_append_edges: n >= 1, M >= 1, PATCH_LIFETIME >= 1 and E >= 0 required"),
    ("dpvo_append_edges", (P, P, P, E, None, 2, 4, 13, P, P, P, None), -1, "dpvo_append_edges: null operand"),
    ("dpvo_append_edges", (None, P, P, E, P, 2, 4, 13, P, P, P, None), -1, "dpvo_append_edges: null operand"),
    # dpvo_scatter_csr(op, dtype, src, outer, E, inner, index, offs, perm, groups, max_groups, eps, out, out_rows,
    #                  argmax, stream)
    ("dpvo_scatter_csr", (4, 1, P, 1, E, D, P, P, P, P, 4, 0.0, P, 4, P, None), -1,
     "dpvo_scatter_csr: op must be 0 (sum), 1 (mean), 2 (max) or 3 (softmax)"),
    ("dpvo_scatter_csr", (0, 1, P, 1, -1, D, P, P, P, P, 4, 0.0, P, 4, P, None), -1, "dpvo_scatter_csr: bad sizes"),
    ("dpvo_scatter_csr", (0, 1, P, 1, 1 << 31, D, P, P, P, P, 4, 0.0, P, 4, P, None), -1,
     "dpvo_scatter_csr: at most 2^31 - 1 elements along the scatter dim"),
    ("dpvo_scatter_csr", (2, 1, P, 1, E, D, P, P, P, P, 4, 0.0, P, 4, None, None), -1,
     "dpvo_scatter_csr: scatter max needs the argmax output"),
    ("dpvo_scatter_csr", (0, 1, P, 1, E, D, P, None, P, P, 4, 0.0, P, 4, P, None), -1,
     "dpvo_scatter_csr: null operand"),
    ("dpvo_scatter_csr", (0, 99, P, 1, E, D, P, P, P, P, 4, 0.0, P, 4, P, None), -1,
     "dpvo_scatter_csr: unsupported dtype"),
    ("dpvo_scatter_csr", (0, 99, None, 1, E, D, P, P, P, P, 0, 0.0, P, 4, P, None), 0, None),   # max_groups first
]

# size queries: (entry point, arguments, value)
QUERIES = [
    ("dpvo_append_edges_count", (0, 4, 13), -1),
    ("dpvo_append_edges_count", (2, 0, 13), -1),
    ("dpvo_append_edges_count", (2, 4, 0), -1),
    ("dpvo_window_group_by_workspace_bytes", (E, 0), 0),
    ("dpvo_window_group_by_workspace_bytes", (E, 23), 0),
]


def run_cases(lib, pointer):
    """[(entry point, arguments, got, want)] of every case that misses; pointer stands in for P"""
    bad = []
    for name, args, rc, msg in CASES:
        got = getattr(lib, name)(*[pointer if a is P else a for a in args])
        err = lib.dpvo_hot_last_error().decode() if got != 0 else None
        if (got, err) != (rc, msg):
            bad.append((name, args, (got, err), (rc, msg)))
    for name, args, want in QUERIES:
        got = getattr(lib, name)(*args)
        if got != want:
            bad.append((name, args, got, want))
    return bad


def test_bad_calls_fail_in_the_checks_with_the_documented_text():
    import _dpvo_hot
    buf = torch.zeros(WS_BYTES, dtype=torch.uint8, device="cuda")
    keep = buf.clone()
    torch.cuda.synchronize()
    assert run_cases(_dpvo_hot.lib(), buf.data_ptr()) == []
    torch.cuda.synchronize()
    assert torch.equal(buf, keep)      # (no call wrote to its operands)
