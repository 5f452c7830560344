"""Degenerate values that real scans and trained networks produce and random test data never does: exact ties in a
max, an activation input of exactly 0, a channel without variance, a softmax that is one-hot, tied or far beyond the
range of expf, ranges of 0 m or far past the sensor's maximum.

The referee is always a plain float64 computation of the same operation on the CPU (torch float64, or
oracle/ref_numpy.py), never the code under test.  The data is built from small integers wherever a comparison has to be
branch for branch, so that the float32 kernel and the float64 referee meet the SAME ties; what the referee itself does
on a tie is pinned by the unmarked tests, which run without a GPU.

  1. training tail (bn_act_pool.hip)   ties in both pools, u == 0, a gamma = beta = 0 channel, a constant channel
  2. spatial attention (spatial_attn.hip)   saturated, tied and shifted logits, forward and both backward forms
  3. cutout (cutout.hip)               the 0.01 m clamp of the window width, all-zero / all-padding / far scans
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import ref_numpy as R
from test_hip_parity import _torch_attention

gpu = pytest.mark.gpu


def _dev(a):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.cuda()


# ------------------------------------------------------------------------------------------ 1. training tail
MOMENTUM, EPS, SLOPE = 0.1, 1e-5, 0.1
DEAD, CONST = 0, 1            # channel with gamma = beta = 0; channel with y = 0.75 over the whole batch
# (S, C, L, pool): pool 1 = max over pairs, pool 2 = max over the row
TAIL_CASES = [(12, 8, 8, 1), (5, 6, 10, 1), (33, 64, 48, 1), (6, 4, 4, 2), (9, 8, 16, 2), (4, 8, 256, 2)]
# the generator seed of every case: one for which no |u| of a live channel is below 1e-3 (asserted, not filtered), with
# one group and -- where S is even -- with two
TAIL_SEEDS = {(12, 8, 8, 1): 1, (5, 6, 10, 1): 1, (33, 64, 48, 1): 1, (6, 4, 4, 2): 1, (9, 8, 16, 2): 1, (4, 8, 256, 2): 1}
# pool 2: rows (s, c) whose maximum (3.0, above every other entry) is planted at these positions
TAIL_PLANTS = {
    4: [((0, 2), (1, 2)),                  # inside the row's only lane
        ((1, 2), (0, 3)),                  # position 0 against the last
        ((2, 3), (0, 1, 3))],              # three-way
    16: [((0, 2), (5, 6)),                 # inside one lane's four positions
         ((1, 2), (2, 9)),                 # lanes 0 and 2 of the row
         ((2, 3), (0, 15)),                # position 0 against the last
         ((3, 4), (1, 7, 12))],            # three lanes
    256: [((0, 2), (5, 200)),              # lanes 1 and 50: more than 32 apart
          ((1, 2), (0, 255)),              # lanes 0 and 63: every level of the shuffle reduction
          ((2, 3), (130, 131)),            # inside lane 32
          ((3, 4), (3, 140)),              # lanes 0 and 35
          ((0, 5), (66, 129, 255))],       # three lanes, two of them 32 or more from the first
}
# (case, form): "one_shot" groups = 1; "groups2" two statistics groups (S even: the kernel wants equal groups);
# "sync" the four-call global-batch form on two uneven shards
TAIL_RUNS = [(c, f) for c in TAIL_CASES for f in ("one_shot", "sync")] + \
            [(c, "groups2") for c in TAIL_CASES if c[0] % 2 == 0]
TAIL_IDS = ["%dx%dx%d-pool%d-%s" % (c + (f,)) for c, f in TAIL_RUNS]


def _tail_out_shape(S, C, L, pool):
    return (S, C) if pool == 2 else (S, C, L // 2 if pool else L)


@functools.lru_cache(maxsize=None)
def _tail_inputs(S, C, L, pool):
    """float32 CPU tensors of one case (built once, shared, never modified)."""
    rng = np.random.default_rng(TAIL_SEEDS[(S, C, L, pool)])
    y = rng.integers(-2, 3, (S, C, L)).astype(np.float32)
    if pool == 2:
        for (s, c), pos in TAIL_PLANTS[L]:
            y[s, c, list(pos)] = 3.0
    y[:, CONST, :] = 0.75
    gam = rng.uniform(0.5, 1.5, C)
    bet = rng.uniform(0.1, 0.5, C) * rng.choice([-1.0, 1.0], C)
    gam[DEAD] = bet[DEAD] = 0.0
    bet[CONST] = 0.5 * rng.choice([-1.0, 1.0])
    inp = dict(y=y, gam=gam, bet=bet, rm=rng.uniform(-1, 1, C), rv=rng.uniform(0.5, 2.0, C),
               dz=rng.normal(size=_tail_out_shape(S, C, L, pool)))
    return {k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in inp.items()}


def _pool64(a, pool):
    return torch.max(a, 2)[0] if pool == 2 else torch.max_pool1d(a, 2) if pool == 1 else a


@functools.lru_cache(maxsize=None)
def _tail_referee(S, C, L, pool, groups):
    """batch_norm(train) -> leaky_relu(0.1) -> pool in float64 on the CPU, every group with its own statistics, and its
    autograd; also u (the activation's input) and xhat for the preconditions and the closed forms."""
    inp = _tail_inputs(S, C, L, pool)
    y64 = inp["y"].double().requires_grad_(True)
    g64, b64 = inp["gam"].double().requires_grad_(True), inp["bet"].double().requires_grad_(True)
    rm64, rv64 = inp["rm"].double().clone(), inp["rv"].double().clone()
    us, xhs, outs = [], [], []
    for part in y64.chunk(groups, dim=0):
        u = torch.nn.functional.batch_norm(part, rm64, rv64, g64, b64, True, MOMENTUM, EPS)
        us.append(u.detach())
        p = part.detach()
        mean, var = p.mean(dim=(0, 2), keepdim=True), p.var(dim=(0, 2), unbiased=False, keepdim=True)
        xhs.append((p - mean) / torch.sqrt(var + EPS))
        outs.append(_pool64(torch.nn.functional.leaky_relu(u, SLOPE), pool))
    z64 = torch.cat(outs, dim=0)
    z64.backward(inp["dz"].double())
    return dict(z=z64.detach(), u=torch.cat(us), xhat=torch.cat(xhs), dy=y64.grad, dgam=g64.grad, dbet=b64.grad,
                rm=rm64, rv=rv64)


def _first_winner_sums(S, C, L, pool, groups):
    """sum dz and sum dz * xhat over the first element of every pair / row of the DEAD channel, float64."""
    inp, ref = _tail_inputs(S, C, L, pool), _tail_referee(S, C, L, pool, groups)
    dz, xh = inp["dz"].double()[:, DEAD], ref["xhat"][:, DEAD]
    first = xh[:, 0] if pool == 2 else xh[:, 0::2]
    return float(dz.sum()), float((dz * first).sum())


def _check_tail_preconditions(S, C, L, pool, groups):
    inp, ref = _tail_inputs(S, C, L, pool), _tail_referee(S, C, L, pool, groups)
    u = ref["u"]
    live = [c for c in range(C) if c != DEAD]
    assert float(u[:, live].abs().min()) >= 1e-3, (S, C, L, pool, groups, float(u[:, live].abs().min()))
    assert torch.all(u[:, DEAD] == 0.0)                        # exactly: every pair and every row a full tie
    # the constant channel: xhat exactly 0, u = beta up to the residue of torch's own scale / shift form
    assert torch.all(ref["xhat"][:, CONST] == 0.0) and float((u[:, CONST] - inp["bet"][CONST].double()).abs().max()) <= 1e-12
    # equal y give bit-equal u in float64, so the referee meets the ties that the float32 kernel meets
    y, lo = inp["y"], [c for c in range(C) if c not in (DEAD, CONST)]
    same_y, same_u = (y[:, lo, 0::2] == y[:, lo, 1::2]), (u[:, lo, 0::2] == u[:, lo, 1::2])
    assert torch.equal(same_y, same_u)
    if pool == 1:
        assert 0.1 <= float(same_y.float().mean()) <= 0.3     # about a fifth of all pairs tie
    else:
        # the planted rows: a two- or three-way tie at the maximum, and the referee routes it to the first position
        arg = torch.max(torch.nn.functional.leaky_relu(u, SLOPE), 2)[1]
        for (s, c), pos in TAIL_PLANTS[L]:
            assert int((u[s, c] == u[s, c].max()).sum()) == len(pos) and int(arg[s, c]) == pos[0]
            # the whole dz of the row sits on the first maximum: the later ones differ from it by gamma / std * dz
            sg = S // groups
            var = inp["y"][s // sg * sg:(s // sg + 1) * sg, c].double().var(unbiased=False)
            d = ref["dy"][s, c, pos[0]] - ref["dy"][s, c, list(pos[1:])]
            want = float(inp["gam"][c].double() / torch.sqrt(var + EPS)) * float(inp["dz"][s, c])
            assert torch.allclose(d, torch.full_like(d, want), rtol=1e-9, atol=1e-12)


def test_float64_referee_routes_ties_to_the_first_maximum_and_uses_the_slope_at_zero():
    """What the float64 CPU referee does on the degenerate inputs, so that its semantics are pinned as well: a tied
    pair (max_pool1d) and a tied row (torch.max over a dimension) send the gradient to the FIRST maximum, and the
    derivative of leaky_relu at exactly 0 (either sign of zero) is the slope."""
    x = torch.tensor([[[1.0, 1.0, 0.0, 2.0, 2.0, 2.0, -1.0, -1.0]]], dtype=torch.float64, requires_grad=True)
    torch.max_pool1d(x, 2).backward(torch.tensor([[[1.0, 2.0, 3.0, 4.0]]], dtype=torch.float64))
    assert x.grad.flatten().tolist() == [1.0, 0.0, 0.0, 2.0, 3.0, 0.0, 4.0, 0.0]
    r = torch.tensor([[[0.0, 5.0, 1.0, 5.0, 5.0], [7.0, 7.0, 7.0, 7.0, 7.0]]], dtype=torch.float64, requires_grad=True)
    val, idx = torch.max(r, 2)
    assert idx.tolist() == [[1, 0]]
    val.backward(torch.tensor([[2.0, 3.0]], dtype=torch.float64))
    assert r.grad.tolist() == [[[0.0, 2.0, 0.0, 0.0, 0.0], [3.0, 0.0, 0.0, 0.0, 0.0]]]
    z = torch.tensor([0.0, -0.0, 1.0, -1.0], dtype=torch.float64, requires_grad=True)
    torch.nn.functional.leaky_relu(z, SLOPE).backward(torch.ones(4, dtype=torch.float64))
    assert z.grad.tolist() == [SLOPE, SLOPE, 1.0, SLOPE]


@pytest.mark.parametrize("case,form", TAIL_RUNS, ids=TAIL_IDS)
def test_tail_fixtures_meet_their_preconditions(case, form):
    """On the float64 referee's own values: no |u| of a live channel below 1e-3 (so that no branch of the comparison
    hangs on a rounding), the dead channel exactly 0, the constant channel at beta (1e-12), the ties where they were
    planted.  Nothing is filtered out of the comparison; the seeds are fixed so that this holds."""
    _check_tail_preconditions(*case, 2 if form == "groups2" else 1)


def _run_tail(ops, S, C, L, pool, form):
    """The fused tail in one of its forms -> float64 CPU results under the referee's names."""
    inp = {k: _dev(v) for k, v in _tail_inputs(S, C, L, pool).items()}
    y, gam, bet, dz = inp["y"], inp["gam"], inp["bet"], inp["dz"]
    rm, rv = inp["rm"].clone(), inp["rv"].clone()
    if form != "sync":
        groups = 2 if form == "groups2" else 1
        z, mu, istd = ops.bn_lrelu_pool_forward(y, gam, bet, rm, rv, MOMENTUM, EPS, SLOPE, pool, groups=groups)
        dy, dgam, dbet = ops.bn_lrelu_pool_backward(y, dz, gam, bet, mu, istd, SLOPE, pool, groups=groups)
        dgam, dbet = dgam.double(), dbet.double()
    else:
        cut = max(1, S // 3)
        rows = [torch.arange(0, cut).cuda(), torch.arange(cut, S).cuda()]           # two uneven shards
        ys, dzs = [y[r].contiguous() for r in rows], [dz[r].contiguous() for r in rows]
        stat = torch.stack([ops.bn_sync_forward_stats(yk) for yk in ys]).sum(dim=0)  # the all-reduce
        z, dy = torch.empty(_tail_out_shape(S, C, L, pool), device="cuda"), torch.empty_like(y)
        for yk, r in zip(ys, rows):
            rmk, rvk = inp["rm"].clone(), inp["rv"].clone()
            z[r], mu, istd = ops.bn_sync_forward_apply(yk, stat, gam, bet, rmk, rvk, MOMENTUM, EPS, SLOPE, pool)
            rm, rv = rmk, rvk
        back = [ops.bn_sync_backward_reduce(yk, dzk, gam, bet, mu, istd, SLOPE, pool) for yk, dzk in zip(ys, dzs)]
        red = torch.stack([b[0] for b in back]).sum(dim=0)
        dgam = torch.stack([b[1] for b in back]).double().sum(dim=0)
        dbet = torch.stack([b[2] for b in back]).double().sum(dim=0)
        for yk, dzk, r in zip(ys, dzs, rows):
            dy[r] = ops.bn_sync_backward_apply(yk, dzk, gam, bet, mu, istd, red, stat, SLOPE, pool)
    torch.cuda.synchronize()
    got = dict(z=z, istd=istd, rm=rm, rv=rv, dy=dy, dgam=dgam, dbet=dbet)
    return {k: v.double().cpu() for k, v in got.items()}


@gpu
@pytest.mark.parametrize("case,form", TAIL_RUNS, ids=TAIL_IDS)
def test_tail_on_ties_zeros_and_dead_channels(case, form):
    """bn_lrelu_pool_forward / _backward (and the global-batch form) on integer data full of exact ties, with one
    gamma = beta = 0 channel and one constant channel, against the float64 referee at the bars of
    test_bn_lrelu_pool_matches_torch_modules (pairs) and test_bn_lrelu_rowmax_matches_torch (rows).  A tie routed to the
    second maximum, or the derivative 1 instead of the slope at u == 0, moves dy by O(|dz|): four orders above them."""
    from planar_optical_flow_amd import ops
    S, C, L, pool = case
    groups = 2 if form == "groups2" else 1
    _check_tail_preconditions(S, C, L, pool, groups)
    inp, ref = _tail_inputs(S, C, L, pool), _tail_referee(S, C, L, pool, groups)
    got = _run_tail(ops, S, C, L, pool, form)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
    norm = [c for c in range(C) if c != CONST]
    err = lambda a, b: float((a - b).abs().max())
    if pool == 2:
        assert err(got["z"], ref["z"]) <= 2e-5 * float(ref["z"].abs().max())
        gbar = dict(dy=1e-4, dgam=1e-4, dbet=1e-4)
        run_tol = dict(rtol=1e-5, atol=1e-6)
    else:
        assert torch.allclose(got["z"], ref["z"], rtol=1e-5, atol=2e-5)
        gbar = dict(dy=2e-5, dgam=1e-5, dbet=1e-5)
        run_tol = dict(rtol=1e-6, atol=1e-6)
    assert torch.allclose(got["rm"], ref["rm"], **run_tol) and torch.allclose(got["rv"], ref["rv"], **run_tol)
    # dy: the constant channel carries 1/sqrt(eps) = 316 in its scale, so it is held to its own largest entry and
    # every other channel to the largest entry of the others (each no looser than the bar on the whole tensor)
    for chans in (norm, [CONST]):
        scale = max(float(ref["dy"][:, chans].abs().max()), 1.0)
        assert err(got["dy"][:, chans], ref["dy"][:, chans]) <= gbar["dy"] * scale, (chans[0], scale)
    for k in ("dgam", "dbet"):
        assert err(got[k], ref[k]) <= gbar[k] * max(float(ref[k].abs().max()), 1.0), k
    # the gamma = beta = 0 channel: u is exactly 0, every pair and row a full tie, the derivative the slope
    assert torch.all(got["z"][:, DEAD] == 0.0) and torch.all(got["dy"][:, DEAD] == 0.0)
    s_dz, s_dzx = _first_winner_sums(S, C, L, pool, groups)
    assert abs(float(got["dbet"][DEAD]) - SLOPE * s_dz) <= gbar["dbet"] * max(float(ref["dbet"].abs().max()), 1.0)
    assert abs(float(got["dgam"][DEAD]) - SLOPE * s_dzx) <= gbar["dgam"] * max(float(ref["dgam"].abs().max()), 1.0)
    # the constant channel: variance exactly 0
    want_istd = 1.0 / np.sqrt(EPS)
    for g in range(groups):
        assert abs(float(got["istd"][g * C + CONST]) - want_istd) <= 1e-6 * want_istd
    want_rv = (1.0 - MOMENTUM) ** groups * float(inp["rv"][CONST].double())          # updated with 0, once per group
    assert abs(float(got["rv"][CONST]) - want_rv) <= 1e-6 * want_rv


def _segment_batch():
    """Eight detections of 5, 20 and 63 distinct points, far apart, as one point cloud."""
    rng = np.random.default_rng(7)
    sizes = [5, 20, 63, 5, 20, 63, 5, 20]
    centers = np.stack([np.array([10.0 * k, -3.0 + k]) for k in range(len(sizes))])
    pts = np.concatenate([c + rng.uniform(-0.25, 0.25, (n, 2)) for c, n in zip(centers, sizes)])
    return pts, centers, rng.uniform(-3, 3, len(sizes)), sizes


@gpu
def test_box_head_training_step_on_padded_segments():
    """One step up: a box-head training step on a batch as the feeder emits it -- segments of 5, 20 and 63 points
    repeated and padded to 64 rows by ops.segment_inputs, so every row of the PointNet's max over points has its
    maximum 12-13, 3-4 or 1-2 times -- with the HIP units (fused row-max tail) against the torch-module path, at the bar of
    test_drow_training_step_fused_tail_matches_module_path."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "planar_optical_flow_amd"))
    from src.model.get_model import get_model
    from planar_optical_flow_amd import ops
    pts, centers, oris, sizes = _segment_batch()
    x, count = ops.segment_inputs(_dev(pts), _dev(centers), _dev(oris), radius=0.4, input_size=64, min_segment_size=5,
                                  seed=5)
    assert count.tolist() == sizes and tuple(x.shape) == (8, 64, 3)
    for s, n in enumerate(sizes):       # the multiplicities are real: n distinct rows, each at least 64 // n times
        rows, mult = np.unique(x[s].cpu().numpy(), axis=0, return_counts=True)
        assert len(rows) == n and mult.min() >= 64 // n and mult.sum() == 64
    torch.manual_seed(11)
    cfg = {"type": "box_reg", "input_dim": 3, "target_dim": 3, "dropout": 0.0}
    a, b = get_model(cfg).cuda().train(), get_model(cfg).cuda().train()
    b.load_state_dict(a.state_dict())
    a.backbone.hip_train, b.backbone.hip_train = True, False
    tgt = torch.randn(8, 3, device="cuda")
    outs = []
    for m in (a, b):
        pred = m(x)
        loss = m.loss_fn(pred, tgt)
        loss.backward()
        outs.append((pred.detach(), float(loss.detach())))
    assert torch.allclose(outs[0][0], outs[1][0], rtol=1e-3, atol=1e-4)
    assert abs(outs[0][1] - outs[1][1]) <= 1e-3 * abs(outs[1][1]) + 1e-4
    gscale = max(float(p.grad.abs().max()) for p in b.parameters() if p.grad is not None)
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        assert (p.grad is None) == (q.grad is None), n
        if p.grad is not None:
            assert float((p.grad - q.grad).abs().max()) <= 2e-3 * gscale, n
    for (n, p), q in zip(a.named_buffers(), b.buffers()):
        assert torch.allclose(p.double(), q.double(), rtol=1e-4, atol=1e-5), n


# ------------------------------------------------------------------------------------------ 2. spatial attention
ATTN_B, ATTN_F = 2, 64
ATTN_SHAPES = [(N, E, W) for N in (40, 5) for E in (128, 6) for W in (7, 11)]
ATTN_KINDS = ("first_frame", "zero_template", "duplicated_rows", "one_hot", "scaled_shifted")
ATTN_GAP = 104.0        # expf(-104) is 0 in float32 with or without denormals (2^-150 = e^-103.97)


def _attn_alpha(W):
    return 0.5 if W == 11 else 0.3


def _attn_embeddings(kind, N, E):
    """Integer embeddings: every dot product is exact in float32 (and in float64)."""
    rng = np.random.default_rng(100 * N + E + 7 * ATTN_KINDS.index(kind))
    B = ATTN_B
    ints = lambda: rng.integers(-2, 3, (B, N, E)).astype(np.float64)
    amp = 2.0 if E == 128 else 8.0      # |q|^2 = 512 or 384: one step of a logit is more than 150
    q = amp * rng.choice([-1.0, 1.0], (B, 1, E))
    odd = 1.0 + (np.arange(N) % 2).reshape(1, N, 1)            # rows of emb_x differ: q, 2q, q, ...
    if kind == "first_frame":                                   # the template is a clone of the features
        ex = ints()
        return ex, ex.copy()
    if kind == "zero_template":                                 # all logits equal
        return ints(), np.zeros((B, N, E))
    if kind == "duplicated_rows":                               # template rows q in a sea of -q: 2- and 3-way ties
        et = np.broadcast_to(-q, (B, N, E)).copy()
        marks = ((10, 12, 25, 26, 27), (3, 4, 20, 22, 24)) if N == 40 else ((1, 3), (0, 1, 2))
        for b in range(B):
            et[b, list(marks[b])] = q[b]
        return q * odd, et
    if kind == "one_hot":                                       # logits m_j |q|^2, m_j distinct inside every window
        m = np.stack([((5 * np.arange(N) + 3 * b) % 16) - 8.0 for b in range(B)]).reshape(B, N, 1)
        return q * odd, m * q
    if kind == "scaled_shifted":                                # logits of +-10^6: nothing without max-subtraction
        return 64.0 * ints(), 64.0 * ints() - 1000.0
    raise ValueError(kind)


def _band_valid(N, W):
    """[N, W] bool: slot k of row i is a distinct in-window column (not a clamped duplicate)."""
    j = np.arange(N)[:, None] - W // 2 + np.arange(W)[None, :]
    return (j >= 0) & (j <= N - 1)


def _gband_only(ex, et, g_band, W):
    """The gradients of sum(band * g_band) alone, float64: what d_emb_x / d_emb_t must be when the softmax is
    saturated (p (1 - p) = 0 everywhere)."""
    B, N, E = ex.shape
    cols = np.clip(np.arange(N)[:, None] - W // 2 + np.arange(W)[None, :], 0, N - 1)
    dex = np.einsum("bik,bike->bie", g_band, et[:, cols])
    det = np.zeros_like(et)
    for k in range(W):
        for i in range(N):
            det[:, cols[i, k]] += g_band[:, i, k, None] * ex[:, i]
    return dex, det


@functools.lru_cache(maxsize=None)
def _attn_case(kind, N, E, W):
    """Inputs (float32 numpy) and every float64 referee result of one case, computed once."""
    B, F, alpha = ATTN_B, ATTN_F, _attn_alpha(W)
    ex64, et64 = _attn_embeddings(kind, N, E)
    rng = np.random.default_rng(9000 + 10 * N + E + W)
    x, t = rng.normal(0, 1, (B, N, F)).astype(np.float32), rng.normal(0, 1, (B, N, F)).astype(np.float32)
    g_out, g_band = rng.normal(0, 1, (B, N, F)).astype(np.float32), rng.normal(0, 1, (B, N, W)).astype(np.float32)
    c = dict(ex=ex64.astype(np.float32), et=et64.astype(np.float32), x=x, t=t, g_out=g_out, g_band=g_band, alpha=alpha)
    assert np.array_equal(c["ex"].astype(np.float64), ex64) and np.array_equal(c["et"].astype(np.float64), et64)
    c["out64"], c["band64"] = R.spatial_attention(ex64, et64, x.astype(np.float64), t.astype(np.float64), alpha, W)
    x16, t16 = x.astype(np.float16), t.astype(np.float16)
    c["x16"], c["t16"] = x16, t16
    c["out64_h"], _ = R.spatial_attention(ex64, et64, x16.astype(np.float64), t16.astype(np.float64), alpha, W)
    # the softmax over the distinct in-window columns, float64, and its exact form where the logits are separated
    valid = _band_valid(N, W)[None]
    s = np.where(valid, c["band64"], -np.inf)
    mx = s.max(axis=-1, keepdims=True)
    e = np.exp(s - mx)
    c["prob64"] = e / e.sum(axis=-1, keepdims=True)
    tie = valid & (c["band64"] == mx)
    c["separated"] = np.all(~valid | tie | (c["band64"] <= mx - ATTN_GAP), axis=-1)        # [B, N]
    c["prob_exact"] = (tie.astype(np.float32) / tie.sum(axis=-1, keepdims=True).astype(np.float32)).astype(np.float32)
    c["ties"] = tie.sum(axis=-1)
    c["one_hot"] = bool((c["ties"] == 1).all() and c["separated"].all())       # every row saturated onto one column
    # float64 autograd of the plain torch formulation
    leaves = [torch.from_numpy(a.astype(np.float64)).requires_grad_(True) for a in (ex64, et64, x, t)]
    out_r, band_r = _torch_attention(*leaves, alpha, W)
    assert out_r.dtype == torch.float64 and np.array_equal(band_r.detach().numpy(), c["band64"])
    np.testing.assert_allclose(out_r.detach().numpy(), c["out64"], rtol=1e-12, atol=1e-12)
    ((out_r * torch.from_numpy(g_out).double()).sum() + (band_r * torch.from_numpy(g_band).double()).sum()).backward()
    c["grads64"] = [a.grad.numpy() for a in leaves]
    c["gband_only"] = _gband_only(ex64, et64, g_band.astype(np.float64), W)
    return c


def _attn_exact(kind, E):
    """Cases whose every row is separated: prob is an exact rational (1/k on the ties, 0 elsewhere)."""
    return kind != "first_frame" or E == 128


@pytest.mark.parametrize("N,E,W", ATTN_SHAPES)
@pytest.mark.parametrize("kind", ATTN_KINDS)
def test_attention_fixtures_meet_their_preconditions(kind, N, E, W):
    """On the float64 referee: finite everywhere (also at logits of +-10^6), the rows separated by more than expf's
    range where the test claims an exact prob, the ties, one-hot rows and saturation that each case is there for."""
    c = _attn_case(kind, N, E, W)
    assert np.isfinite(c["out64"]).all() and np.isfinite(c["prob64"]).all() and all(np.isfinite(g).all() for g in c["grads64"])
    np.testing.assert_allclose(c["prob64"].sum(-1), 1.0, rtol=0, atol=1e-12)
    if _attn_exact(kind, E):
        assert c["separated"].all()
        np.testing.assert_allclose(c["prob64"], c["prob_exact"], rtol=0, atol=1e-7)      # float32 of 1/3: 1e-8 off
    valid = _band_valid(N, W)
    if kind == "first_frame" and E == 128:
        diag = c["band64"][:, :, W // 2]
        assert diag.min() >= 150 and (c["ties"] == 1).all() and np.array_equal(c["prob_exact"][:, :, W // 2], np.ones_like(diag))
        # saturated to the last bit in the referee too: the merge is alpha x + (1 - alpha) tmpl
        a = c["alpha"]
        assert np.array_equal(c["out64"], a * c["x"].astype(np.float64) + (1.0 - a) * c["t"].astype(np.float64))
    if kind == "zero_template":
        assert np.array_equal(c["prob_exact"], np.broadcast_to((valid / valid.sum(-1, keepdims=True).astype(np.float32))
                                                               .astype(np.float32), c["prob_exact"].shape))
        if W == 11 and N == 40:
            assert c["prob_exact"][0, 0, 5] == np.float32(1) / np.float32(6) and c["prob_exact"][0, 20, 0] == np.float32(1) / np.float32(11)
    if kind == "duplicated_rows":
        assert {2, 3} <= set(np.unique(c["ties"]).tolist())
    if kind == "one_hot":
        assert (c["ties"] == 1).all()
    if kind == "scaled_shifted":
        big = 1e6 if E == 128 else 1e5
        assert np.abs(c["band64"]).max() >= big
    assert c["one_hot"] == (kind == "one_hot" or (kind == "first_frame" and E == 128)) or kind == "scaled_shifted"
    if c["one_hot"]:
        # where every row is one-hot, autograd's d_emb is the g_band term alone
        for g, want in zip(c["grads64"][:2], c["gband_only"]):
            np.testing.assert_allclose(g, want, rtol=0, atol=1e-9 * max(np.abs(want).max(), 1.0))


@gpu
@pytest.mark.parametrize("N,E,W", ATTN_SHAPES)
@pytest.mark.parametrize("kind", ATTN_KINDS)
def test_attention_forward_under_saturation(kind, N, E, W):
    """ops.spatial_attention (float32 and float16 storage) on saturated, tied and shifted logits: band bit for bit (the
    dot products are exact), prob an exact rational wherever the logits are separated by more than expf's range and 0
    on clamped duplicates, out at the bar of the golden tests."""
    from planar_optical_flow_amd import ops
    c = _attn_case(kind, N, E, W)
    out, band, prob = ops.spatial_attention(_dev(c["ex"]), _dev(c["et"]), _dev(c["x"]), _dev(c["t"]), c["alpha"], W)
    out, band, prob = out.cpu().numpy(), band.cpu().numpy(), prob.cpu().numpy()
    assert np.isfinite(out).all() and np.isfinite(band).all() and np.isfinite(prob).all()
    assert np.array_equal(band.astype(np.float64), c["band64"])
    np.testing.assert_allclose(prob.sum(-1), 1.0, rtol=0, atol=1e-6)
    assert np.all(prob[:, ~_band_valid(N, W)] == 0.0)                                  # clamped duplicates: no weight
    np.testing.assert_allclose(prob, c["prob64"], rtol=0, atol=1e-6)
    if _attn_exact(kind, E):
        assert np.array_equal(prob, c["prob_exact"])
    np.testing.assert_allclose(out, c["out64"], rtol=1e-4, atol=1e-5)
    # float16 storage: the same band and prob, out = the float32 result on the same inputs rounded once
    x16, t16 = _dev(c["x16"]), _dev(c["t16"])
    oh, bh, ph = ops.spatial_attention(_dev(c["ex"]), _dev(c["et"]), x16, t16, c["alpha"], W)
    of, _, _ = ops.spatial_attention(_dev(c["ex"]), _dev(c["et"]), x16.float(), t16.float(), c["alpha"], W)
    assert oh.dtype == torch.float16
    assert np.array_equal(bh.cpu().numpy(), band) and np.array_equal(ph.cpu().numpy(), prob)
    assert torch.equal(oh, of.to(torch.float16))
    np.testing.assert_allclose(oh.float().cpu().numpy(), c["out64_h"], rtol=2e-3, atol=2e-3)


@gpu
@pytest.mark.parametrize("N,E,W", ATTN_SHAPES)
@pytest.mark.parametrize("kind", ATTN_KINDS)
def test_attention_backward_under_saturation(kind, N, E, W):
    """Both backward forms on the same cases against float64 autograd of the plain torch formulation: every gradient
    within 2e-4 of the referee's largest entry (test_spatial_attention_backward_vs_autograd), the fused form against the
    two-pass form as in test_spatial_attention_backward_fused_equals_two_pass, and -- where every row is one-hot --
    d_emb equal to the g_band term alone."""
    from planar_optical_flow_amd import ops
    c = _attn_case(kind, N, E, W)
    ex, et, t = _dev(c["ex"]), _dev(c["et"]), _dev(c["t"])
    go, gb = _dev(c["g_out"]), _dev(c["g_band"])
    _, _, prob = ops.spatial_attention(ex, et, _dev(c["x"]), t, c["alpha"], W)
    res = {}
    for fused in (False, True):
        got = ops.spatial_attention_backward(ex, et, t, prob, go, gb, c["alpha"], W, fused=fused)
        res[fused] = got
        for name, a, want in zip(("d_emb_x", "d_emb_t", "d_x", "d_tmpl"), got, c["grads64"]):
            a = a.double().cpu().numpy()
            assert np.isfinite(a).all(), (name, fused)
            err, scale = float(np.abs(a - want).max()), float(np.abs(want).max())
            assert err <= 2e-4 * scale, (name, fused, err, scale)
        if c["one_hot"]:
            for name, a, want in zip(("d_emb_x", "d_emb_t"), got[:2], c["gband_only"]):
                err, scale = float(np.abs(a.double().cpu().numpy() - want).max()), float(np.abs(want).max())
                assert err <= 2e-4 * scale, (name, fused, err, scale)
    assert torch.equal(res[True][2], res[False][2]) and torch.equal(res[True][3], res[False][3])
    for a, b in zip(res[True][:2], res[False][:2]):
        assert float((a - b).abs().max()) <= 2e-5 * max(float(b.abs().max()), 1.0)


# ------------------------------------------------------------------------------------------ 3. cutout
CUT_GRIDS = {"n90": (1.0, 90), "n180": (0.5, 180)}
CUT_PARAMS = {
    "area12": dict(fixed=True, area_mode=True, num_cutout_pts=12, window_width=1.0, window_depth=0.5),
    "stride2": dict(fixed=False, area_mode=False, num_cutout_pts=8, stride=2),
    "wide56": dict(fixed=True, area_mode=True, num_cutout_pts=56, window_width=1.66, centered=False),
}
CUT_SCANS = ("zeros", "padding", "tiny", "far")
CUT_B, CUT_T = 2, 3
TINY = np.array([0.0, 1e-40, 1e-3, 0.00999, 0.01, np.nextafter(np.float32(0.01), np.float32(1.0)), 0.02], dtype=np.float32)
FAR = np.array([65.0, 1e4], dtype=np.float32)


def _cut_kw(name):
    kw = dict(stride=1, centered=True, fixed=False, window_width=1.66, window_depth=1.0, num_cutout_pts=48,
              padding_val=29.99, area_mode=False)
    kw.update(CUT_PARAMS[name])
    return kw


@functools.lru_cache(maxsize=None)
def _cut_scans(kind, N):
    """[B, T, N] float32.  The planted beams sit at even and at odd indices of every scan row (with stride 2 only the
    even ones are window centres; the odd ones are neighbours inside other windows), and once as a run of three."""
    if kind == "zeros":
        return np.zeros((CUT_B, CUT_T, N), dtype=np.float32)
    if kind == "padding":
        return np.full((CUT_B, CUT_T, N), 29.99, dtype=np.float32)
    rng = np.random.default_rng(600 + N + (0 if kind == "tiny" else 1))
    scans = rng.uniform(0.5, 25.0, (CUT_B, CUT_T, N)).astype(np.float32)
    vals = TINY if kind == "tiny" else FAR
    for b in range(CUT_B):
        for t in range(CUT_T):
            even = rng.choice(np.arange(0, N, 2), len(vals), replace=False)
            odd = rng.choice(np.arange(1, N, 2), len(vals), replace=False)
            scans[b, t, even] = vals
            scans[b, t, odd] = vals
            r0 = int(rng.integers(0, N - 3))
            scans[b, t, r0:r0 + 3] = vals[(b + t) % len(vals)]
    return scans


@functools.lru_cache(maxsize=None)
def _cut_oracle(grid, params, kind):
    inc, N = CUT_GRIDS[grid]
    phi = R.laser_phi(np.radians(inc), N)
    return [R.cutout(s, phi, atan_mode="cr", return_debug=True, **_cut_kw(params)) for s in _cut_scans(kind, N)]


@pytest.mark.parametrize("kind", CUT_SCANS)
@pytest.mark.parametrize("params", list(CUT_PARAMS))
@pytest.mark.parametrize("grid", list(CUT_GRIDS))
def test_cutout_oracle_is_defined_on_the_sentinel_scans(grid, params, kind):
    """The oracle (the reference's operations in NumPy) stays finite on every sentinel scan, treats every range below
    0.01 m as 0.01 m, and gives one value everywhere on an all-padding scan (up to the rounding of 29.99)."""
    inc, N = CUT_GRIDS[grid]
    kw = _cut_kw(params)
    scans = _cut_scans(kind, N)
    for b, (want, dbg) in enumerate(_cut_oracle(grid, params, kind)):
        assert np.isfinite(want).all()
        if kw["area_mode"]:
            # the 0.01 m windows span the whole field of view: area-sampled, up to 30 raw points per output
            assert 1 <= dbg["s_area"] <= 30 if kind in ("zeros", "tiny") else dbg["s_area"] >= 0
        if kind == "padding":
            # one value, up to the float32 rounding of 29.99: the beams carry float32(29.99), the samples outside the
            # field of view the float64 padding value
            assert np.ptp(want) <= 1e-6
        if kind in ("zeros", "tiny"):
            # the clamp: with every range below 0.01 m raised to 0.01 m the windows (inds_ct_low) are the same
            raised = np.where(scans[b] < np.float32(0.01), np.float32(0.01), scans[b])
            _, d2 = R.cutout(raised, R.laser_phi(np.radians(inc), N), atan_mode="cr", return_debug=True, **kw)
            assert np.array_equal(dbg["lo"], d2["lo"])
            # ... and it is this constant that matters: a clamp at 0.02 m gives other windows
            raised = np.where(scans[b] < np.float32(0.02), np.float32(0.02), scans[b])
            _, d3 = R.cutout(raised, R.laser_phi(np.radians(inc), N), atan_mode="cr", return_debug=True, **kw)
            assert not np.array_equal(dbg["lo"], d3["lo"])
    if kind == "tiny":
        assert (scans < np.float32(0.01)).sum() >= 4 * CUT_B * CUT_T and (scans == np.float32(0.01)).any()


@gpu
@pytest.mark.parametrize("kind", CUT_SCANS)
@pytest.mark.parametrize("params", list(CUT_PARAMS))
@pytest.mark.parametrize("grid", list(CUT_GRIDS))
def test_cutout_clamp_and_sentinel_scans(grid, params, kind):
    """Values, inds_ct_low and the area factor bit-exact against the oracle (as test_cutout_bit_exact_vs_oracle) on
    all-zero and all-padding scans, on ranges at and below the 0.01 m clamp of the window width, and on ranges far
    beyond the sensor's maximum; the float32 value path at the fuzz test's bar and the float16 output at the bar of
    test_cutout_float16_storage on the same inputs."""
    from planar_optical_flow_amd import ops
    inc, N = CUT_GRIDS[grid]
    kw = _cut_kw(params)
    scans = _cut_scans(kind, N)
    tab = ops.phi_table(np.radians(inc), N)
    got, dbg = ops.cutout(_dev(scans), tab, return_debug=True, **kw)
    fast = ops.cutout(_dev(scans), tab, exact_values=False, **kw)
    half = ops.cutout(_dev(scans), tab, out_dtype=torch.float16, **kw)
    torch.cuda.synchronize()
    lo = dbg["lo"].cpu().numpy()
    for b, (want, wd) in enumerate(_cut_oracle(grid, params, kind)):
        assert np.array_equal(lo[b], wd["lo"]), "inds_ct_low must be bit-exact"
        if kw["area_mode"]:
            assert int(dbg["s_area"][b].item()) == wd["s_area"]
        assert np.array_equal(got[b].cpu().numpy(), want)
        assert np.array_equal(half[b].cpu().numpy(), want.astype(np.float16))
    assert bool(torch.isfinite(got).all())
    if kind == "padding":
        assert float(got.max() - got.min()) <= 1e-6             # every output identical (see the oracle's test)
    assert half.dtype == torch.float16 and torch.equal(half, got.to(torch.float16))
    err = (fast - got).abs().max().item()
    bar = 2e-5 * max(1.0, 1.0 / kw["window_depth"]) * (30.0 if not kw["centered"] else 1.0)
    print("float32 value path: max |fast - exact| = %.3e (bar %.1e)" % (err, bar))
    assert err <= bar, (err, bar)
