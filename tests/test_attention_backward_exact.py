"""The attention backward (A10 training, csrc/spatial_attn.hip) on data where it has one right answer.

The backward entry points take the softmax weights ``prob`` as an INPUT and are linear algebra from there on.  With
small-integer embeddings, gradients and template rows, weights that are multiples of 1/8 and alpha in {0.5, 0.25}
every intermediate is a dyadic rational that float32 holds exactly, so any correct summation order gives the float64
result bit for bit.  This file (no GPU needed) holds

  * ``referee``: the backward in NumPy, written from the index sets (clip / valid), in the dtype of its inputs;
  * its tie to float64 torch autograd of the plain formulation (``test_hip_parity._torch_attention``);
  * ``CASES``: every window, and the sizes at which the kernels change path (tests/test_attention_backward_exact_gpu.py
    runs both device forms on each of them and asks for equality);
  * the proof, from the referee alone, that every accumulated sum of every case fits float32's 24 bits;
  * what the cases are for, from the host-only launch plan;
  * ``FLIPS``: wrong variants of the referee, each of which some case must tell from the right one.
"""
import collections
import functools
import math

import numpy as np
import pytest
import torch

Case = collections.namedtuple("Case", "group B N E F W alpha seed support")
GRAD_NAMES = ("d_emb_x", "d_emb_t", "d_x", "d_tmpl")


def window_of(W):
    """The reference uses int(window / 2) neighbours each side: an even window behaves as window + 1."""
    hw = int(W / 2)
    return hw, 2 * hw + 1


def band_index(N, W):
    """(cols, valid) [N, w]: the clamped column of slot k of row i, and whether the unclamped column is in range."""
    hw, w = window_of(W)
    ju = np.arange(N)[:, None] - hw + np.arange(w)[None]
    return np.clip(ju, 0, N - 1), (ju >= 0) & (ju <= N - 1)


# ---------------------------------------------------------------- the referee
FLIPS = {
    "run at j = 0 one short": "the outermost slot of a clamp run onto column 0 is left out of d_emb_t",
    "run at j = N - 1 one short": "the outermost slot of a clamp run onto column N - 1 is left out of d_emb_t",
    "duplicates dropped from d_emb_t": "only unclamped slots reach d_emb_t",
    "out-of-range slots given their dp": "dp is the dot product with the clamped row instead of 0",
    "d_tmpl takes clamped slots": "d_tmpl is scattered through the clamped columns",
    "last four columns of F dropped": "dp is contracted over F - 4 columns",
    "column 128 of E dropped": "d_emb_x and d_emb_t lose embedding column 128",
    "g_band ignored on clamped slots": "dsim gets g_band on unclamped slots only",
    "s over all slots of dp": "s sums prob times the unmasked dp while dsim uses the masked one",
}
# the flips that only weights on clamped slots can show: the forward writes 0 there, the backward masks by index
NEED_OFF_SUPPORT = ("out-of-range slots given their dp", "d_tmpl takes clamped slots", "s over all slots of dp")


def referee(ex, et, tmpl, prob, g_out, g_band, alpha, W, flip=None, sums=None):
    """-> (d_emb_x, d_emb_t, d_x, d_tmpl, dsim) in the dtype of ``ex`` (float64, or float32 to show that nothing
    rounds).  ``g_band`` None is 0.  ``flip``: one of FLIPS.  ``sums``: a dict that receives, per accumulated
    quantity, (q, a): every term of its sums is a multiple of 2^-q and a is the largest sum of |terms|."""
    assert flip is None or flip in FLIPS, flip
    dt = ex.dtype
    B, N, E = ex.shape
    F = tmpl.shape[2]
    hw, w = window_of(W)
    cols, valid = band_index(N, W)
    a, oma = dt.type(alpha), dt.type(1.0 - alpha)
    gb = np.zeros((B, N, w), dt) if g_band is None else g_band
    if flip == "g_band ignored on clamped slots":
        gb = gb * valid[None].astype(dt)

    def note(name, q, mag):
        if sums is not None:
            old = sums.get(name, (0, 0.0))
            sums[name] = (max(old[0], q), max(old[1], float(mag.max()) if mag.size else 0.0))

    # dp[i, k] = (1 - alpha) <g[i], tmpl[i - hw + k]> on the slots whose unclamped column is in range
    Fd = F - 4 if flip == "last four columns of F dropped" else F
    rows_t = tmpl[:, cols, :Fd]                                            # [B, N, w, F]
    dp_all = oma * np.einsum("bif,bikf->bik", g_out[..., :Fd], rows_t)
    dp = np.where(valid[None], dp_all, dt.type(0))
    if flip == "out-of-range slots given their dp":
        dp = dp_all
    if sums is not None:
        note("dp", _q(oma) + _q(g_out) + _q(tmpl),
             oma * np.einsum("bif,bikf->bik", np.abs(g_out), np.abs(rows_t)) * valid[None])
    # softmax backward of each row, plus the gradient that arrives through ``band``
    s = np.einsum("bik,bik->bi", prob, dp_all if flip == "s over all slots of dp" else dp)
    dsim = prob * (dp - s[..., None]) + gb
    if sums is not None:
        note("s", _q(prob) + _q(dp), np.einsum("bik,bik->bi", np.abs(prob), np.abs(dp)))
        note("dsim", max(_q(prob) + max(_q(dp), _q(s)), _q(gb)),
             np.abs(prob * dp) + np.abs(prob * s[..., None]) + np.abs(gb))
    # d emb_x[i] = sum_k dsim[i, k] emb_t[cols[i, k]];  d emb_t[cols[i, k]] += dsim[i, k] emb_x[i], duplicates kept
    d_emb_x = np.einsum("bik,bike->bie", dsim, et[:, cols])
    d_emb_t = np.zeros_like(et)
    mag_t = np.zeros_like(et)
    run = np.zeros((B, N, N), dt)             # [b, j, i]: sum of |dsim[i, k]| over the slots of row i that land on j
    for i in range(N):
        for k in range(w):
            if flip == "duplicates dropped from d_emb_t" and not valid[i, k]:
                continue
            if flip == "run at j = 0 one short" and k == 0 and i - hw < 0:
                continue
            if flip == "run at j = N - 1 one short" and k == w - 1 and i + hw > N - 1:
                continue
            d_emb_t[:, cols[i, k]] += dsim[:, i, k, None] * ex[:, i]
            if sums is not None:
                mag_t[:, cols[i, k]] += np.abs(dsim[:, i, k, None] * ex[:, i])
                run[:, cols[i, k], i] += np.abs(dsim[:, i, k])
    if flip == "column 128 of E dropped" and E > 128:
        d_emb_x[..., 128] = 0
        d_emb_t[..., 128] = 0
    if sums is not None:
        note("d_emb_x", _q(dsim) + _q(et), np.einsum("bik,bike->bie", np.abs(dsim), np.abs(et[:, cols])))
        note("d_emb_t", _q(dsim) + _q(ex), mag_t)
        note("d_emb_t run", _q(dsim), run)
    # d x = alpha g;  d tmpl[i - hw + k] += (1 - alpha) prob[i, k] g[i] on the unclamped slots
    d_x = a * g_out
    d_tmpl = np.zeros_like(tmpl)
    mag_d = np.zeros_like(tmpl)
    for i in range(N):
        for k in range(w):
            if valid[i, k] or flip == "d_tmpl takes clamped slots":
                d_tmpl[:, cols[i, k]] += oma * prob[:, i, k, None] * g_out[:, i]
                if sums is not None:
                    mag_d[:, cols[i, k]] += np.abs(oma * prob[:, i, k, None] * g_out[:, i])
    if sums is not None:
        note("d_tmpl", _q(oma) + _q(prob) + _q(g_out), mag_d)
    return d_emb_x, d_emb_t, d_x, d_tmpl, dsim


def _q(v):
    """The smallest q with v * 2^q integral in every entry."""
    v = np.asarray(v, np.float64)
    for q in range(0, 64):
        if np.array_equal(np.ldexp(v, q), np.rint(np.ldexp(v, q))):
            return q
    raise AssertionError("not dyadic")


# ---------------------------------------------------------------- the cases
def _cases():
    out = []

    def add(group, B, N, E, F, W, support="valid"):
        n = len(out)
        out.append(Case(group, B, N, E, F, W, (0.5, 0.25)[n % 2], 7000 + n, support))

    # every window: the two ends of the scan on the same rows (N = 1, 2, N <= hw + 1), one window, the 16-point tile
    # and unit boundaries and a last unit of one point; window 10 must behave as 11
    for W in (1, 3, 5, 7, 9, 11, 13, 15):
        for N in sorted({1, 2, W // 2 + 1, W, 16, 17, 33}):
            add("windows", 2, N, 6, 20, W)
    for N in (2, 6, 17):
        add("windows", 2, N, 6, 20, 10)
    # embedding width: below, at and one past the 128-column chunk of attn_demb_kernel, a second chunk that is whole
    for E in (1, 4, 127, 128, 129, 132, 256, 260):
        add("E", 3, 19, E, 8, 11)
    # gradient width: one float4, a partial 16-float step, the register blocks of kDsU steps (64), one wave's columns
    # (256), one workgroup's (512) and a third workgroup (1028), each with the size before and after
    for F in (4, 12, 60, 64, 68, 124, 128, 132, 252, 256, 260, 508, 512, 516, 1028):
        add("F", 3, 21, 8, F, 7)
    for F in (12, 260, 1028):
        add("F", 3, 21, 8, F, 15)
    add("batch", 5, 49, 128, 260, 15)
    # the batch alone fills the chip: both walks take the whole scan per lane
    for W in (3, 11):
        add("batch", 3072, 40, 4, 4, W)
    # 2, 6 and 10 units of 16 points: the last workgroup of four waves is not full
    for W in (3, 7, 15):
        for B in (1, 3, 5):
            add("batch", B, 17, 6, 20, W)
    # 136 points: the merge walk ends in segments of 5, the fused walk in segments of 9, both with one point left over
    for W in (3, 15):
        add("batch", 1, 136, 4, 4, W)
    # weights on clamped slots: the forward never writes them, the backward masks by index and must not lean on that
    for W, N in ((3, 17), (11, 5), (15, 17), (15, 33)):
        add("off-support", 2, N, 6, 20, W, support="all")
    return tuple(out)


CASES = _cases()
GROUPS = ("windows", "E", "F", "batch", "off-support")


def case_id(c):
    return "%s B%d N%d E%d F%d W%d a%g%s" % (c.group, c.B, c.N, c.E, c.F, c.W, c.alpha,
                                              "" if c.support == "valid" else " all-slots")


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """Float64 (ex, et, tmpl, prob, g_out, g_band): integers, and rows of ``prob`` that split 8/8 over the slots."""
    c = case
    rng = np.random.default_rng(c.seed)
    hw, w = window_of(c.W)
    amp = 2 if c.F <= 132 else 1
    ex = rng.integers(-2, 3, (c.B, c.N, c.E)).astype(np.float64)
    et = rng.integers(-2, 3, (c.B, c.N, c.E)).astype(np.float64)
    tmpl = rng.integers(-amp, amp + 1, (c.B, c.N, c.F)).astype(np.float64)
    g_out = rng.integers(-amp, amp + 1, (c.B, c.N, c.F)).astype(np.float64)
    g_band = rng.integers(-3, 4, (c.B, c.N, w)).astype(np.float64)
    _, valid = band_index(c.N, c.W)
    prob = np.zeros((c.B, c.N, w))
    for i in range(c.N):
        slots = np.flatnonzero(valid[i]) if c.support == "valid" else np.arange(w)
        prob[:, i, slots] = rng.multinomial(8, np.full(len(slots), 1.0 / len(slots)), size=c.B) / 8.0
    for a in (ex, et, tmpl, prob, g_out, g_band):
        a.setflags(write=False)
    return ex, et, tmpl, prob, g_out, g_band


@functools.lru_cache(maxsize=None)
def expected(case, with_band):
    """The referee's float64 (d_emb_x, d_emb_t, d_x, d_tmpl) of a case, with g_band given or None."""
    ex, et, tmpl, prob, g_out, g_band = case_inputs(case)
    res = referee(ex, et, tmpl, prob, g_out, g_band if with_band else None, case.alpha, case.W)[:4]
    for a in res:
        a.setflags(write=False)
    return res


def test_case_set():
    assert 100 <= len(CASES) <= 150 and len(set(CASES)) == len(CASES)
    assert {c.group for c in CASES} == set(GROUPS)
    assert {c.W for c in CASES if c.group == "windows"} == {1, 3, 5, 7, 9, 10, 11, 13, 15}
    assert {c.alpha for c in CASES} == {0.5, 0.25}
    for c in CASES:
        ex, et, tmpl, prob, g_out, g_band = case_inputs(c)
        _, valid = band_index(c.N, c.W)
        assert np.array_equal(prob.sum(-1), np.ones((c.B, c.N))) and np.array_equal(prob * 8, np.rint(prob * 8))
        if c.support == "valid":
            assert not prob[:, ~valid].any()                    # clamped slots are exactly 0, as the forward writes them
        else:
            assert prob[:, ~valid].any()
        assert max(np.abs(ex).max(), np.abs(et).max()) <= 2 and np.abs(g_band).max() <= 3
        assert max(np.abs(tmpl).max(), np.abs(g_out).max()) <= (2 if c.F <= 132 else 1)


# ---------------------------------------------------------------- the referee is the reference formulation
AUTOGRAD_SHAPES = (  # B, N, E, F, W, alpha, g_band given
    (2, 1, 5, 8, 7, 0.5, True),          # one point: both ends of the scan are the same row
    (2, 3, 6, 4, 11, 0.3, False),        # N < hw
    (1, 9, 130, 12, 5, 0.7, True),       # E > 128
    (2, 17, 7, 20, 15, 0.25, False),
    (3, 12, 4, 8, 10, 0.5, True),        # an even window
    (1, 16, 3, 4, 1, 0.9, True),
    (2, 6, 8, 16, 3, 0.5, False),
)


@pytest.mark.parametrize("shape", AUTOGRAD_SHAPES, ids=lambda s: "B%d N%d E%d F%d W%d" % s[:5])
def test_referee_equals_float64_autograd(shape):
    """Random float64 data, weights from the masked softmax of the band: the referee equals float64 autograd of the
    plain torch formulation to 1e-12 of each tensor's largest entry."""
    from test_hip_parity import _torch_attention
    B, N, E, F, W, alpha, with_band = shape
    rng = np.random.default_rng(100 + N + E)
    ex, et = rng.standard_normal((B, N, E)), rng.standard_normal((B, N, E))
    x, tmpl, g_out = (rng.standard_normal((B, N, F)) for _ in range(3))
    hw, w = window_of(W)
    g_band = rng.standard_normal((B, N, w)) if with_band else None
    leaves = [torch.from_numpy(a).requires_grad_(True) for a in (ex, et, x, tmpl)]
    out, band = _torch_attention(*leaves, alpha, W)
    loss = (out * torch.from_numpy(g_out)).sum()
    if with_band:
        loss = loss + (band * torch.from_numpy(g_band)).sum()
    loss.backward()
    cols, valid = band_index(N, W)
    sim = np.einsum("bie,bike->bik", ex, et[:, cols])
    assert np.abs(sim - band.detach().numpy()).max() <= 1e-12 * np.abs(sim).max()
    e = np.where(valid[None], np.exp(sim - np.where(valid[None], sim, -np.inf).max(-1, keepdims=True)), 0.0)
    prob = e / e.sum(-1, keepdims=True)
    got = referee(ex, et, tmpl, prob, g_out, g_band, alpha, W)
    want = [leaves[0].grad, leaves[1].grad, leaves[2].grad, leaves[3].grad]
    for name, a, b in zip(GRAD_NAMES, got, want):
        b = b.numpy()
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), (name, np.abs(a - b).max(), np.abs(b).max())


# ---------------------------------------------------------------- nothing rounds
@functools.lru_cache(maxsize=None)
def widest_sums():
    """{quantity: (bits, case id)}: log2 of the largest sum of |terms| in units of the terms' grid, over all cases and
    both g_band settings."""
    worst = {}
    for c in CASES:
        ex, et, tmpl, prob, g_out, g_band = case_inputs(c)
        for with_band in (True, False):
            sums = {}
            referee(ex, et, tmpl, prob, g_out, g_band if with_band else None, c.alpha, c.W, sums=sums)
            for name, (q, mag) in sums.items():
                bits = q + math.log2(mag) if mag > 0 else 0.0
                if bits > worst.get(name, (-1.0, None))[0]:
                    worst[name] = (bits, case_id(c))
    return worst


def test_every_sum_fits_float32():
    """For dp, s, dsim, the d_emb_x sums, the d_emb_t sums and their folded runs, and d_tmpl, of every case: with q the
    smallest exponent that makes every term integral, sum |terms| * 2^q < 2^24 -- so no partial sum, in any order,
    leaves float32's integers."""
    worst = widest_sums()
    assert set(worst) == {"dp", "s", "dsim", "d_emb_x", "d_emb_t", "d_emb_t run", "d_tmpl"}
    for name, (bits, where) in sorted(worst.items()):
        print("%-12s widest sum %.1f bits (%s)" % (name, bits, where))
        assert bits < 24, (name, bits, where)


@pytest.mark.parametrize("group", GROUPS)
def test_float32_evaluation_gives_the_float64_bits(group):
    for c in CASES:
        if c.group != group:
            continue
        inp = case_inputs(c)
        for with_band in (True, False):
            f32 = [a.astype(np.float32) for a in inp]
            got = referee(*f32[:5], f32[5] if with_band else None, c.alpha, c.W)[:4]
            for name, a, b in zip(GRAD_NAMES, got, expected(c, with_band)):
                assert a.dtype == np.float32 and np.array_equal(a.astype(np.float64), b), (case_id(c), with_band, name)


# ---------------------------------------------------------------- what the cases are for
@pytest.fixture(scope="module")
def ops():
    from planar_optical_flow_amd import build, _lib
    build.build(verbose=False)
    _lib.load()
    from planar_optical_flow_amd import ops as _ops
    return _ops


def test_what_the_cases_are_for(ops):
    """From the host-only launch plan: the segments both walks cut the cases into, the column blocks whose partials
    the fused form sums, the chunks of the embedding, the units of the band product."""
    seen = {"merge": set(), "fused": set()}
    ncb, units_mod4 = set(), set()
    for c in CASES:
        hw, w = window_of(c.W)
        for walk, L in zip(("merge", "fused"), ops.spatial_attention_plan(c.B, c.N, c.F)):
            last = c.N - (math.ceil(c.N / L) - 1) * L
            seen[walk] |= {"whole scan" if L == c.N else "segments", "last of %d" % last}
            if L < c.N and L < hw:
                seen[walk].add("shorter than hw")
        ncb.add(2 * ((c.F // 4 + 127) // 128))
        units_mod4.add(c.B * ((c.N + 15) // 16) % 4)
    for walk in ("merge", "fused"):
        assert {"whole scan", "segments", "last of 1"} <= seen[walk], (walk, sorted(seen[walk]))
    assert "shorter than hw" in seen["merge"]
    assert ops.spatial_attention_plan(2, 33, 20)[0] == 5          # 5-point segments under the 7-point halo of W = 15
    assert any(c == Case("windows", 2, 33, 6, 20, 15, c.alpha, c.seed, "valid") for c in CASES)
    for B, W in ((3072, 3), (3072, 11)):
        assert ops.spatial_attention_plan(B, 40, 4) == (40, 40)
    assert ops.spatial_attention_plan(1, 136, 4) == (5, 9) and 136 % 5 == 1 and 136 % 9 == 1
    assert ncb == {2, 4, 6}
    assert {1, 2} <= units_mod4                                   # last workgroups of one and of two live waves
    assert all(c.B * ((c.N + 15) // 16) % 4 == 2 for c in CASES if c.group == "batch" and c.N == 17)
    assert any(c.E % 128 == 1 and c.E > 128 for c in CASES)       # an E chunk of one column
    assert any(c.E > 128 and c.E % 128 == 0 for c in CASES)       # two whole chunks
    assert any(c.N == 1 for c in CASES)                           # j = 0 and j = N - 1 are the same row
    assert any(1 < c.N <= window_of(c.W)[0] for c in CASES)       # N <= hw: every window spans the whole scan
    assert any(c.N % 16 == 1 and c.N > 16 for c in CASES) and any(c.N == 16 for c in CASES)
    assert {c.F % 16 for c in CASES} >= {0, 4, 12}                # whole steps and both partial steps of the band product


# ---------------------------------------------------------------- the cases separate the errors these kernels can have
@pytest.mark.parametrize("flip", sorted(FLIPS))
def test_every_error_is_held_by_a_case(flip):
    changed = []
    for c in CASES:
        ex, et, tmpl, prob, g_out, g_band = case_inputs(c)
        for with_band in (True, False):
            got = referee(ex, et, tmpl, prob, g_out, g_band if with_band else None, c.alpha, c.W, flip=flip)[:4]
            names = [n for n, a, b in zip(GRAD_NAMES, got, expected(c, with_band)) if not np.array_equal(a, b)]
            if names:
                changed.append((case_id(c), with_band, names))
            if flip in NEED_OFF_SUPPORT and c.support == "valid":
                assert not names, (flip, case_id(c))              # invisible while clamped slots carry no weight
        if len(changed) >= 3:
            break
    assert changed, flip
    print("%s: changes %s" % (flip, changed[:3]))
