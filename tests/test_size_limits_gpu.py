"""Kernels at the sizes their own comments call the limit, and one step past it.

1. nms_kernel, the NMS form for scans of 513..4096 points: every padded size and LDS step (the opt-in above 64 KB of
   dynamic LDS from N = 1025), distinct and tied scores, distances at the threshold, non-finite centres and min_dist,
   the refusal at 4097 and a small call right after an opt-in call -- against the float64 oracle.
2. band_corr_bwd_kernel for n = 255..512 (the opt-in from n = 432 with the widest band) against float64 autograd of the
   reference formulation, exact on integer data; the refusal at 513.
3. segment_inputs_kernel / segment_resample_kernel at the candidate cap (4096): the kernels are deterministic, so every
   output ROW is predicted from a NumPy port of the kernels' hash (the "shuffle") and compared exactly.
4. The other stated limits in one table: the at-limit call against the reference of its nearest existing test, one
   past refused with the shape code, no stale error, output buffers untouched.
5. Odometry association of a sample whose odometry range is empty (NaN and -1, nothing read), and the constructor's
   refusal of a sequence without odometry rows.

Tests without the gpu mark check, on the host, the preconditions the GPU tests rely on (and assert again): a fixture
change cannot quietly stop covering a branch.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import ref_numpy as R
from planar_optical_flow_amd import synth
from test_dispatch_gpu import _DR, T

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from planar_optical_flow_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _ops


def _refused(fn, *untouched):
    """fn() raises PofError with the shape code, leaves no stale HIP error behind and writes none of the buffers in
    `untouched` (pre-filled with 7)."""
    from planar_optical_flow_amd import _lib
    _lib.take_stale_error()
    with pytest.raises(_lib.PofError) as e:
        fn()
    assert e.value.code == _lib.POF_E_SHAPE
    assert _lib.take_stale_error() == 0
    torch.cuda.synchronize()
    for buf in untouched:
        assert bool((buf == 7).all())


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------- 1. NMS, the form for N > 512
# N -> (angle increment in degrees, dynamic LDS of nms_kernel in bytes)
NMS_SIZES = {513: (0.5, 36 << 10), 1024: (0.25, 36 << 10), 1025: (0.25, 72 << 10), 2048: (0.125, 72 << 10),
             2049: (0.125, 144 << 10), 3600: (0.1, 144 << 10), 4096: (0.0625, 144 << 10)}
NMS_MIN_DIST = (0.2, 0.5, 1.5)


def _nms_lds(N):
    """Dynamic LDS of nms_kernel: three float64 and three int32 arrays over the size padded to a power of two."""
    npad = 1
    while npad < N:
        npad <<= 1
    return npad * (3 * 8 + 3 * 4)


def _nms_oracle(scan, phi, cls, reg, md, stable=False):
    with np.errstate(all="ignore"):
        return R.nms_predicted_center(scan, phi, cls[:, None], reg, md, stable_ties=stable)


def _nms_assert(got, want, where):
    """got: (xy, cls, num, inst) host arrays of one scan; want: the oracle's triple.  Counts, instance ids and kept
    scores exact, centres within 1e-12 * max(1, |xy|max); matching inf / NaN centres are equal."""
    xy, dc, num, inst = got
    wxy, wcls, winst = want
    m = int(num)
    assert m == len(wxy), where
    assert np.array_equal(inst, winst), where
    assert np.array_equal(dc[:m], wcls[:, 0]), where
    fin = np.abs(wxy[np.isfinite(wxy)])
    scale = max(1.0, float(fin.max())) if fin.size else 1.0
    np.testing.assert_allclose(xy[:m], wxy, rtol=0, atol=1e-12 * scale, equal_nan=True, err_msg=str(where))


def _nms_run(ops, scans, tab, cls, reg, md):
    out = ops.nms_predicted_center(T(scans), tab, T(cls), T(reg), md)
    xy, dc, num, inst = (a.cpu().numpy() for a in out)
    return [(xy[b], dc[b], num[b], inst[b]) for b in range(len(scans))]


def _nms_random(N, B, inc, seed):
    rng = np.random.default_rng(seed)
    sb = synth.make_batch(seed=seed + 1, B=B, T=1, N=N, angle_inc=np.radians(inc))
    cls = rng.permutation(B * N).reshape(B, N).astype(np.float64) / (B * N)          # distinct scores
    reg = rng.normal(0, 0.3, (B, N, 2))
    return sb.scans[:, 0], cls, reg


@pytest.mark.gpu
@pytest.mark.parametrize("N", sorted(NMS_SIZES))
def test_nms_long_form_sizes(ops, N):
    """nms_kernel at the first size it serves, either side of both padded-size steps, the README's 3600-point scanner
    and the limit (8 scan flags per thread).  From N = 1025 the launch needs the opt-in for more than 64 KB of LDS."""
    inc, lds = NMS_SIZES[N]
    assert 512 < N <= 4096 and _nms_lds(N) == lds and (lds > 64 << 10) == (N >= 1025)
    B = 3 if N <= 1025 else 2
    md = NMS_MIN_DIST[sorted(NMS_SIZES).index(N) % 3]
    scans, cls, reg = _nms_random(N, B, inc, 4000 + N)
    phi = R.laser_phi(np.radians(inc), N)
    tab = ops.phi_table(np.radians(inc), N)
    got = _nms_run(ops, scans, tab, cls, reg, md)
    for b in range(B):
        _nms_assert(got[b], _nms_oracle(scans[b], phi, cls[b], reg[b], md), (N, md, b))
    # tied scores, as a saturated sigmoid gives them: the kernel's order is total, equal scores by descending index
    tied = np.round(cls * 7) / 7
    tied[:, ::3] = 1.0
    got = _nms_run(ops, scans, tab, tied, reg, md)
    for b in range(B):
        _nms_assert(got[b], _nms_oracle(scans[b], phi, tied[b], reg[b], md, stable=True), (N, md, b, "tied"))


@functools.lru_cache(maxsize=None)
def _threshold_case():
    """3600-point scans (0.1 degree) that each hold 16 well separated pairs of centres whose distance is min_dist give
    or take 0..5 float32 steps of one range, every other centre far from them; scan 0 also has a huge coordinate.
    -> scans, cls, reg, pairs (b, i, j), the oracle's result per scan."""
    rng = np.random.default_rng(99)
    N, md, B, P = 3600, 0.5, 3, 16
    phi = R.laser_phi(np.radians(0.1), N)
    scans = np.full((B, N), 25.0, np.float32)
    reg = np.zeros((B, N, 2))
    cls = np.tile(np.linspace(0.4, 0.1, N), (B, 1))            # distinct, low everywhere else
    pairs = []
    for b in range(B):
        for p in range(P):
            q = b * P + p
            i = 100 + 210 * p + int(rng.integers(0, 50))
            j = i + int(rng.integers(1, 6))                    # a few beams apart
            Rr = float(np.float32(rng.uniform(4.0, 20.0)))
            dl = phi[j] - phi[i]
            disc = md * md - (Rr * np.sin(dl)) ** 2
            assert disc > 0
            r = np.float32(Rr * np.cos(dl) + np.sqrt(disc))    # |c_i - c_j| = min_dist up to the rounding of r
            for _ in range((q // 2) % 6):
                r = np.nextafter(r, np.float32(np.inf if q % 2 else 0.0))
            scans[b, i], scans[b, j] = np.float32(Rr), r
            cls[b, i], cls[b, j] = 0.9 - 1e-3 * p, 0.8 - 1e-3 * p
            pairs.append((b, i, j))
    scans[0, 3] = np.float32(3.0e6)
    want = [_nms_oracle(scans[b], phi, cls[b], reg[b], md) for b in range(B)]
    return scans, cls, reg, md, pairs, want


def _threshold_sides(pairs, want):
    """(pairs the oracle merges, pairs it keeps apart): centre j carries i's instance id iff dist < min_dist."""
    merged = sum(1 for b, i, j in pairs if want[b][2][j] == want[b][2][i])
    return merged, len(pairs) - merged


def test_nms_threshold_fixture_has_pairs_on_both_sides():
    scans, cls, reg, md, pairs, want = _threshold_case()
    merged, apart = _threshold_sides(pairs, want)
    assert merged >= 8 and apart >= 8, (merged, apart)
    xy = np.array(R.polar_to_xy(scans.astype(np.float64), R.laser_phi(np.radians(0.1), 3600)[None]))
    for b, i, j in pairs:
        d = np.hypot(*(xy[:, b, i] - xy[:, b, j]))
        assert abs(d - md) <= 8 * np.spacing(np.float32(scans[b, j])), (b, i, j, d)      # inside the band of a few steps
        assert want[b][2][i] > 0 and want[b][2][j] > 0


@pytest.mark.gpu
def test_nms_long_form_distances_at_the_threshold(ops):
    """nms_kernel compares sqrt(dx * dx + dy * dy) < min_dist itself (the one-wave form compares squares against a
    host-side bound): kept set and instance ids equal the oracle's float64 decisions on both sides of the threshold."""
    scans, cls, reg, md, pairs, want = _threshold_case()
    merged, apart = _threshold_sides(pairs, want)
    assert merged >= 1 and apart >= 1
    got = _nms_run(ops, scans, ops.phi_table(np.radians(0.1), 3600), cls, reg, md)
    for b in range(len(scans)):
        _nms_assert(got[b], want[b], ("threshold", b))


NONFINITE_BEAMS = (5, 77, 140, 201, 333, 440)       # present at N = 450 and N = 3600


@functools.lru_cache(maxsize=None)
def _nonfinite_case(N):
    """Two scans with six ranges set to inf / NaN; those points carry the lowest scores of the scan, distinct, so the
    oracle's visiting order -- and with it its kept set -- does not depend on where a sort puts a NaN."""
    inc = 0.1 if N == 3600 else 0.5
    scans, cls, reg = _nms_random(N, 2, inc, 8800 + N)
    scans = scans.copy()
    phi = R.laser_phi(np.radians(inc), N)
    for b in range(2):
        for k, beam in enumerate(NONFINITE_BEAMS):
            scans[b, beam] = np.float32(np.nan if (k + b) % 2 else np.inf)
            cls[b, beam] = -(k + 1.0) / N
    want = [_nms_oracle(scans[b], phi, cls[b], reg[b], 0.5) for b in range(2)]
    return scans, cls, reg, inc, want


def _check_nonfinite_preconditions(N):
    scans, cls, reg, inc, want = _nonfinite_case(N)
    phi = R.laser_phi(np.radians(inc), N)
    beams = list(NONFINITE_BEAMS)
    rest = np.setdiff1d(np.arange(N), beams)
    for b in range(2):
        assert not np.isfinite(scans[b, beams]).any() and np.isfinite(scans[b, rest]).all()
        assert np.isinf(scans[b, beams]).any() and np.isnan(scans[b, beams]).any()
        assert len(np.unique(cls[b])) == N and cls[b, beams].max() < cls[b, rest].min()
        # inf * cos / sin of the beam angle has a definite sign: no beam on an axis
        assert np.abs(np.cos(phi[beams])).min() > 1e-3 and np.abs(np.sin(phi[beams])).min() > 1e-3
        wxy, wcls, winst = want[b]
        # the rule: such a centre is kept, suppresses nothing and keeps instance id 0
        assert np.count_nonzero(~np.isfinite(wxy).all(axis=1)) == len(beams)
        assert np.array_equal(wcls[-len(beams):, 0], np.sort(cls[b, beams])[::-1])
        assert (winst[beams] == 0).all() and (winst[rest] > 0).all()
        fin = _nms_oracle(scans[b][rest], phi[rest], cls[b][rest], reg[b][rest], 0.5)
        assert np.array_equal(fin[0], wxy[:-len(beams)]) and np.array_equal(fin[2], winst[rest])


@pytest.mark.parametrize("N", [450, 3600])
def test_nms_oracle_is_defined_on_the_nonfinite_scans(N):
    _check_nonfinite_preconditions(N)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [450, 3600])
def test_nms_nonfinite_centres_both_forms(ops, N):
    """A centre with an infinite or NaN coordinate is within min_dist of nothing, itself included: it is kept,
    suppresses nothing and its point keeps instance id 0 -- in nms_wave_kernel (N = 450) and nms_kernel (N = 3600)."""
    _check_nonfinite_preconditions(N)
    scans, cls, reg, inc, want = _nonfinite_case(N)
    got = _nms_run(ops, scans, ops.phi_table(np.radians(inc), N), cls, reg, 0.5)
    for b in range(2):
        _nms_assert(got[b], want[b], (N, b))
        assert (got[b][3][list(NONFINITE_BEAMS)] == 0).all()


@pytest.mark.gpu
def test_nms_infinite_min_dist_takes_the_long_form(ops):
    """min_dist = inf has no squared bound, so N = 450 runs nms_kernel: the top score suppresses every other centre."""
    N = 450
    scans, cls, reg = _nms_random(N, 3, 0.5, 31)
    phi = R.laser_phi()
    got = _nms_run(ops, scans, ops.phi_table(), cls, reg, np.inf)
    for b in range(3):
        _nms_assert(got[b], _nms_oracle(scans[b], phi, cls[b], reg[b], np.inf), ("inf", b))
        assert int(got[b][2]) == 1 and (got[b][3] == 1).all() and got[b][1][0] == cls[b].max()


@pytest.mark.gpu
def test_nms_refuses_4097_and_recovers(ops):
    N = 4097
    scans, cls, reg = _nms_random(N, 1, 0.05, 32)
    tab = ops.phi_table(np.radians(0.05), N)
    _refused(lambda: ops.nms_predicted_center(T(scans), tab, T(cls), T(reg), 0.5))
    scans, cls, reg = _nms_random(450, 2, 0.5, 33)
    got = _nms_run(ops, scans, ops.phi_table(), cls, reg, 0.5)
    for b in range(2):
        _nms_assert(got[b], _nms_oracle(scans[b], R.laser_phi(), cls[b], reg[b], 0.5), ("after refusal", b))


@pytest.mark.gpu
def test_nms_small_launch_after_an_opt_in_launch(ops):
    """N = 4096 raises the kernel's dynamic LDS limit to 144 KB; the N = 700 launch (36 KB) that follows on the same
    kernel still equals the oracle."""
    assert _nms_lds(4096) > 64 << 10 >= _nms_lds(700)
    scans, cls, reg = _nms_random(4096, 1, 0.0625, 34)
    ops.nms_predicted_center(T(scans), ops.phi_table(np.radians(0.0625), 4096), T(cls), T(reg), 1.5)
    scans, cls, reg = _nms_random(700, 2, 0.5, 35)
    got = _nms_run(ops, scans, ops.phi_table(np.radians(0.5), 700), cls, reg, 0.2)
    phi = R.laser_phi(np.radians(0.5), 700)
    for b in range(2):
        _nms_assert(got[b], _nms_oracle(scans[b], phi, cls[b], reg[b], 0.2), ("after opt-in", b))


# ---------------------------------------------------------------- 2. band-correlation backward, n up to 512
BWD_CONFIGS = [(33, 5, 7), (40, 3, 5), (64, 1, 7), (3, 3, 2), (1, 1, 0)]          # (C, kernel size, max displacement)


def _bwd_lds(n, K, md):
    """Dynamic LDS of band_corr_bwd_kernel: the band image [n][W] and the output gradient [D][n], float32."""
    return n * ((2 * (md + 2 * (K // 2)) + 1) + (2 * md + 1)) * 4


def _bwd_autograd64(f1, f2, gout, K, md):
    from test_hip_parity import _torch_fusion
    l1, l2 = f1.double().requires_grad_(True), f2.double().requires_grad_(True)
    (_torch_fusion(l1, l2, K, md) * gout.double()).sum().backward()
    return l1.grad, l2.grad


@pytest.mark.gpu
@pytest.mark.parametrize("n", [255, 256, 257, 431, 432, 450, 511, 512])
def test_band_correlation_backward_up_to_512(ops, n):
    """band_corr_bwd_kernel around the 32-position tile edges at 256 and 512, at the Prototype's n = 450 and either
    side of n = 432, from where the widest band needs more than 64 KB of LDS: float64 autograd of the reference
    formulation on integer data (every sum exact in float32), bit for bit."""
    gen = torch.Generator(device="cpu").manual_seed(700 + n)
    for C, K, md in BWD_CONFIGS:
        if (C, K, md) == (33, 5, 7):
            assert _bwd_lds(n, K, md) == n * 38 * 4
            assert (n * 38 * 4 > 65536) == (n >= 432)
        else:
            assert _bwd_lds(n, K, md) <= 65536
        f1 = torch.randint(-3, 4, (2, C, n), generator=gen).float().to(DEV)
        f2 = torch.randint(-3, 4, (2, C, n), generator=gen).float().to(DEV)
        gout = torch.randint(-3, 4, (2, 2 * md + 1, n), generator=gen).float().to(DEV)
        d1, d2 = ops.band_correlation_backward(f1, f2, gout, K, md)
        w1, w2 = _bwd_autograd64(f1, f2, gout, K, md)
        assert torch.equal(d1.double(), w1), (n, C, K, md, (d1.double() - w1).abs().max().item())
        assert torch.equal(d2.double(), w2), (n, C, K, md, (d2.double() - w2).abs().max().item())


@pytest.mark.gpu
def test_band_correlation_backward_n450_float_values(ops):
    """The Prototype's training shape at 3600 points (n = 450, C = 64, kernel 3, displacement 5) on normal data
    against float64 autograd, at the bar of test_band_correlation_backward_vs_autograd (rtol 1e-4, atol 1e-4)."""
    gen = torch.Generator(device="cpu").manual_seed(450)
    f1 = torch.randn(2, 64, 450, generator=gen).to(DEV)
    f2 = torch.randn(2, 64, 450, generator=gen).to(DEV)
    gout = torch.randn(2, 11, 450, generator=gen).to(DEV)
    d1, d2 = ops.band_correlation_backward(f1, f2, gout, 3, 5)
    w1, w2 = _bwd_autograd64(f1, f2, gout, 3, 5)
    for got, want in ((d1, w1), (d2, w2)):
        print("band_corr backward n=450: max |err| %.3e, max |grad| %.3e"
              % ((got.double() - want).abs().max().item(), want.abs().max().item()))
        np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=1e-4, atol=1e-4)


@pytest.mark.gpu
def test_band_correlation_backward_refuses_513_and_recovers(ops):
    from planar_optical_flow_amd import _lib, torch_ops  # noqa: F401
    gen = torch.Generator(device="cpu").manual_seed(513)
    f1 = torch.randint(-3, 4, (2, 5, 513), generator=gen).float().to(DEV)
    f2 = torch.randint(-3, 4, (2, 5, 513), generator=gen).float().to(DEV)
    gout = torch.randint(-3, 4, (2, 11, 513), generator=gen).float().to(DEV)
    _refused(lambda: ops.band_correlation_backward(f1, f2, gout, 3, 5))
    # the forward has no such limit; its backward refuses from inside autograd
    l1, l2 = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    out = torch.ops.pof.band_correlation(l1, l2, 3, 5)
    want = R.band_correlation(f1.double().cpu().numpy(), f2.double().cpu().numpy(), 3, 5).astype(np.float32)
    assert np.array_equal(out.detach().cpu().numpy(), want)
    _refused(lambda: (out * gout).sum().backward())
    assert l1.grad is None and l2.grad is None
    # n = 57: the shuffle form, right after the refusals
    f1, f2, gout = f1[:, :, :57].contiguous(), f2[:, :, :57].contiguous(), gout[:, :, :57].contiguous()
    d1, d2 = ops.band_correlation_backward(f1, f2, gout, 3, 5)
    w1, w2 = _bwd_autograd64(f1, f2, gout, 3, 5)
    assert torch.equal(d1.double(), w1) and torch.equal(d2.double(), w2)


# ---------------------------------------------------------------- 3. segment preparation, exact rows
SEG_CAP = 4096
_M32 = np.uint64(0xFFFFFFFF)


def _mix32(h):
    """mix32 of segment_inputs.hip; uint32 arithmetic carried in uint64 and masked after every product."""
    h = np.asarray(h, dtype=np.uint64) & _M32
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & _M32
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & _M32
    return h ^ (h >> np.uint64(16))


def _point_hash(seed, det, idx):
    """point_hash(seed, det, idx) of segment_inputs.hip for an array of point indices: the kernels' shuffle."""
    inner = _mix32(np.uint64(det) * np.uint64(0x7F4A7C15) + _mix32(np.uint64(int(seed) & 0xFFFFFFFF)))
    return _mix32(np.asarray(idx, dtype=np.uint64) * np.uint64(0x9E3779B9) + inner)


def _hash_order(seed, det, idx):
    """idx in the order the kernels sort it: ascending (hash, index)."""
    idx = np.asarray(idx, dtype=np.int64)
    return idx[np.lexsort((idx, _point_hash(seed, det, idx)))]


def _row_sources(n, M):
    """Sorted position each of the M rows takes from a segment of n points: a random subset when n > M, else
    np.repeat(seg, M // n) followed by its own first rows."""
    j = np.arange(M)
    if n > M:
        return j
    rep = M // n
    return np.where(j < n * rep, j // rep, (j - n * rep) // rep)


def test_hash_port_is_a_permutation_source():
    h = _point_hash(12345, 3, np.arange(4096))
    assert h.dtype == np.uint64 and int(h.max()) < 1 << 32 and len(np.unique(h)) == 4096
    for seed, det in ((12345, 4), (12346, 3)):                   # another batch position or seed: another order
        assert not np.array_equal(np.argsort(_point_hash(seed, det, np.arange(4096))), np.argsort(h))
    # mix32 is the 32-bit finaliser with these constants: spot values worked by hand in Python integers
    def mix(v):
        v ^= v >> 16
        v = (v * 0x85EBCA6B) & 0xFFFFFFFF
        v ^= v >> 13
        v = (v * 0xC2B2AE35) & 0xFFFFFFFF
        return v ^ (v >> 16)
    for seed, det, idx in ((0, 0, 0), (7, 2, 4095), (0xFFFFFFFF, 65535, 123456)):
        want = mix((idx * 0x9E3779B9 + mix((det * 0x7F4A7C15 + mix(seed)) & 0xFFFFFFFF)) & 0xFFFFFFFF)
        assert int(_point_hash(seed, det, [idx])[0]) == want


# launches of segment_inputs: name -> (input_size, min_segment_size, seed, candidate counts, repeated clusters)
# a repeated cluster is a second detection on the same centre: another position in the batch, another hash
SEG_LAUNCHES = {
    "m64": (64, 5, 20240, (4, 5, 7, 50, 63, 64, 65, 4095, 4096, 4097, 5000), (2, 9)),
    "m64_min1": (64, 1, 77, (1, 7, 50), (1,)),
    "m1024": (1024, 5, 2 ** 32 + 5, (4097, 5000, 1023, 1024, 1025, 50), (0,)),
}
SEG_RADIUS = 0.4


@functools.lru_cache(maxsize=None)
def _inputs_case(name, D):
    """Points with exactly counts[k] of them within 0.3 of centre k (radius 0.4) and every other point metres away,
    in shuffled order, Np no multiple of 256 -> everything the launch needs and the predicted output."""
    M, min_size, seed, counts, repeats = SEG_LAUNCHES[name]
    rng = np.random.default_rng(len(name) * 100 + D)
    ctr = np.array([[12.0 * k + 1.3, 3.7 * (k % 2) - 0.9, 0.25][:D] for k in range(len(counts))])
    pts = []
    for k, n in enumerate(counts):
        v = rng.normal(size=(n, D))
        v *= (rng.uniform(0.02, 0.3, n) / np.linalg.norm(v, axis=1))[:, None]
        pts.append(ctr[k] + v)
    pts.append(rng.uniform(900.0, 950.0, (37, D)))
    pts = np.concatenate(pts)
    if len(pts) % 256 == 0:
        pts = np.concatenate([pts, rng.uniform(900.0, 950.0, (1, D))])
    pts = pts[rng.permutation(len(pts))]
    dets = list(range(len(counts))) + list(repeats)
    centers = ctr[dets]
    oris = rng.uniform(-3, 3, len(dets))
    x = np.zeros((len(dets), M, D + 1), np.float32)
    count = np.zeros(len(dets), np.int32)
    mask = np.zeros((len(dets), len(pts)), bool)
    thinned = {}
    for s, k in enumerate(dets):
        dist = np.linalg.norm(pts - centers[s], axis=1)
        assert ((dist < 0.31) | (dist > 5.0)).all()                   # nobody near the rim: no rounding question
        mask[s] = dist <= SEG_RADIUS
        cand = np.nonzero(mask[s])[0]
        n = count[s] = len(cand)
        assert n == counts[k]
        if n < min_size:
            continue
        if n > SEG_CAP:      # the kernel's pre-thinning: candidates whose hash is below 2^32 * 3072 / n
            thr = np.uint64(int(4294967296.0 * (3072.0 / n)))
            cand = cand[_point_hash(seed, s, cand) < thr]
            thinned[s] = len(cand)
        src = _hash_order(seed, s, cand)[_row_sources(n, M)]
        x[s, :, :D] = (pts[src] - centers[s]).astype(np.float32)
        x[s, :, D] = np.float32(oris[s])
    return dict(M=M, min_size=min_size, seed=seed, pts=pts, centers=centers, oris=oris, dets=dets, x=x, count=count,
                mask=mask, thinned=thinned)


def _check_inputs_preconditions(name, D):
    c = _inputs_case(name, D)
    M, counts = c["M"], SEG_LAUNCHES[name][3]
    assert len(c["pts"]) % 256 != 0 and len(c["dets"]) > len(counts) >= 3
    over = [s for s in range(len(c["dets"])) if c["count"][s] > SEG_CAP]
    assert sorted(c["thinned"]) == over and (len(over) > 0) == (max(counts) > SEG_CAP)
    for s in over:
        # the M smallest hashes overall are the M smallest of the thinned list only while it holds M..4096 entries
        assert M <= c["thinned"][s] <= SEG_CAP, (name, s, c["thinned"][s])
    # the same centre at two batch positions: different rows, each predicted on its own
    for s in range(len(counts), len(c["dets"])):
        first = c["dets"][s]
        assert np.array_equal(c["centers"][s], c["centers"][first]) and c["count"][s] == c["count"][first]
        assert not np.array_equal(c["x"][s, :, :D], c["x"][first, :, :D])
    assert len(np.unique(c["pts"].astype(np.float32), axis=0)) == len(c["pts"])       # rows identify their point


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("name", sorted(SEG_LAUNCHES))
def test_segment_inputs_fixture_preconditions(name, D):
    _check_inputs_preconditions(name, D)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("name", sorted(SEG_LAUNCHES))
def test_segment_inputs_exact_rows(ops, name, D):
    """Every row of every detection equals the prediction from the hash order: below min_segment_size (zero rows,
    the count still reported), n = 1, M % n != 0 with repeats, either side of n = M, either side of the 4096
    candidate cap and the pre-thinned lists above it, input_size 64 and 1024 (the largest accepted)."""
    _check_inputs_preconditions(name, D)
    c = _inputs_case(name, D)
    x, count, mask = ops.segment_inputs(T(c["pts"]), T(c["centers"]), T(c["oris"]), radius=SEG_RADIUS,
                                        input_size=c["M"], min_segment_size=c["min_size"], seed=c["seed"],
                                        return_mask=True)
    assert np.array_equal(count.cpu().numpy(), c["count"])
    assert np.array_equal(mask.cpu().numpy(), c["mask"])
    x = x.cpu().numpy()
    for s in range(len(c["dets"])):
        assert np.array_equal(x[s], c["x"][s]), (name, D, s, int(c["count"][s]))
        if c["count"][s] < c["min_size"]:
            assert not x[s].any()


@pytest.mark.gpu
def test_segment_inputs_refuses_input_size_1025(ops):
    c = _inputs_case("m64_min1", 2)
    _refused(lambda: ops.segment_inputs(T(c["pts"]), T(c["centers"]), T(c["oris"]), input_size=1025))


RESAMPLE_LENGTHS = (0, 1, 5, 63, 64, 65, 200, 4095, 4096)
RESAMPLE_SEED = 2 ** 33 + 4242          # the entry point takes the low 32 bits


@functools.lru_cache(maxsize=None)
def _resample_pool(D):
    rng = np.random.default_rng(60 + D)
    off = np.concatenate(([0], np.cumsum(RESAMPLE_LENGTHS))).astype(np.int32)
    pts = rng.uniform(-3, 3, (int(off[-1]), D))
    assert len(np.unique(pts.astype(np.float32), axis=0)) == len(pts)
    return pts, off, rng.uniform(-1, 1, (len(RESAMPLE_LENGTHS), D)), rng.uniform(-3, 3, len(RESAMPLE_LENGTHS))


def _predict_resample(D, M, drop, with_extra):
    """-> (x, count, dropped point rows per segment) of segment_resample on _resample_pool(D)."""
    pts, off, ctr, extra = _resample_pool(D)
    Wd = D + (1 if with_extra else 0)
    x = np.zeros((len(RESAMPLE_LENGTHS), M, Wd), np.float32)
    count = np.zeros(len(RESAMPLE_LENGTHS), np.int32)
    gone = []
    for s, n_all in enumerate(RESAMPLE_LENGTHS):
        dropped = int(n_all * drop)                       # int(len(input) * random_drop)
        n = count[s] = n_all - dropped
        order = _hash_order(RESAMPLE_SEED, s, np.arange(n_all))
        gone.append(pts[off[s] + order[:dropped]])        # the head of the hash order is what the drop removes
        if n <= 0:
            continue
        src = off[s] + order[dropped:][_row_sources(n, M)]
        x[s, :, :D] = (pts[src] - ctr[s]).astype(np.float32)
        if with_extra:
            x[s, :, D] = np.float32(extra[s])
    return x, count, gone


def test_resample_prediction_counts():
    for drop in (0.0, 0.25, 0.99):
        x, count, gone = _predict_resample(2, 64, drop, False)
        assert [int(c) for c in count] == [n - int(n * drop) for n in RESAMPLE_LENGTHS]
        assert count[0] == 0 and (count[1:] >= 1).all()
        assert [len(g) for g in gone] == [int(n * drop) for n in RESAMPLE_LENGTHS]
    assert int(0.99 * 4096) == 4055 and int(0.25 * 4095) == 1023


@pytest.mark.gpu
@pytest.mark.parametrize("M", [64, 1024])
@pytest.mark.parametrize("D", [2, 3])
def test_segment_resample_exact_rows(ops, D, M):
    """pof_segment_resample on its own: segments from empty to the 4096 cap in one CSR, three drop rates, with and
    without the extra column.  count = n_all - int(n_all * drop), the head of the hash order never appears, every row
    equals the prediction, an empty segment gives zero rows."""
    pts, off, ctr, extra = _resample_pool(D)
    for drop in (0.0, 0.25, 0.99):
        for with_extra in (True, False):
            want, wcount, gone = _predict_resample(D, M, drop, with_extra)
            x, count = ops.segment_resample(T(pts), T(off), T(ctr), T(extra) if with_extra else None,
                                            random_drop=drop, input_size=M, seed=RESAMPLE_SEED)
            x, count = x.cpu().numpy(), count.cpu().numpy()
            assert x.shape == want.shape
            assert np.array_equal(count, wcount), (drop, with_extra)
            for s, n_all in enumerate(RESAMPLE_LENGTHS):
                where = (D, M, drop, with_extra, n_all)
                assert np.array_equal(x[s], want[s]), where
                if count[s] == 0:
                    assert not x[s].any(), where
                seen = {r.tobytes() for r in x[s, :, :D]}
                assert not any((g - ctr[s]).astype(np.float32).tobytes() in seen for g in gone[s]), where


@pytest.mark.gpu
def test_segment_resample_refuses_4097(ops):
    from planar_optical_flow_amd import _lib
    from planar_optical_flow_amd.src.data_handle.jrdb_dataset import JRDBBoxRegressionDataset
    pts, off, ctr, extra = _resample_pool(2)
    _refused(lambda: ops.segment_resample(T(pts), T(off), T(ctr), None, input_size=64, max_segment=4097))
    # a data set that holds a 4097-point segment: the batch is an error, not rows of zeros
    rng = np.random.default_rng(4097)
    frame = {"segments": [rng.normal(0, 0.2, (4097, 2)), rng.normal(0, 0.2, (40, 2))],
             "boxes": np.array([[0.0, 0.0, 0.8, 0.6, 0.3], [2.0, 1.0, 0.8, 0.6, -0.4]]),
             "dets_center": np.array([[0.05, -0.02], [2.02, 1.01]])}
    cfg = {"input_size": 64, "is_3d": False, "min_segment_size": 5,
           "augmentation_kwargs": {"use_data_augmentation": False, "rot_max": 0.0, "dim_max": 0.0, "dist_max": 0.0,
                                   "random_drop": 0.0}}
    ds = JRDBBoxRegressionDataset("val", cfg, [frame], rng=np.random.default_rng(0))
    assert len(ds) == 2
    with pytest.raises(_lib.PofError) as e:
        ds.get_batch([1, 0])
    assert e.value.code == _lib.POF_E_SHAPE


# ---------------------------------------------------------------- 4. the other stated limits
@pytest.mark.gpu
def test_stump_search_limit(ops):
    """n = 2048 samples against the oracle (as test_stump_search_fuzz_against_oracle); 2049 refused."""
    from planar_optical_flow_amd import _lib
    from planar_optical_flow_amd.src.depracted.model.adaboost_person_det import BoostedFeatureDetector
    rng = np.random.default_rng(2048)
    n, D = 2049, 3
    X = np.round(rng.normal(size=(n, D)) * 3, 1)
    Y = np.where(rng.normal(size=n) + X[:, 0] > 0, 1.0, -1.0)
    Y[0], Y[-2], Y[-1] = 1.0, -1.0, -1.0
    Xd, Yd = T(X), T(Y)
    ints, thetas = BoostedFeatureDetector()._search(Xd[:2048].contiguous(), Yd[:2048].contiguous(), None, 2048)
    for d in range(D):
        th, err = R.stump_thresholds(X[:2048, d], Y[:2048])
        assert len(th) > 0 and ints[2, d] == len(th)
        assert ints[0, d] == err.min() and ints[1, d] == err.max()
        assert thetas[0, d] == th[np.argmin(err)] and thetas[1, d] == th[np.argmax(err)]
    oi = torch.full((3, D), 7, dtype=torch.int32, device=DEV)
    ot = torch.full((2, D), 7.0, dtype=torch.float64, device=DEV)
    _refused(lambda: _lib.call("pof_stump_search", Xd.data_ptr(), Yd.data_ptr(), n, None, n, D, oi[0].data_ptr(),
                               ot[0].data_ptr(), oi[1].data_ptr(), ot[1].data_ptr(), oi[2].data_ptr(), _stream()),
             oi, ot)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_drow_heads_limit(ops, dtype):
    """n_cls = 6 (8 outputs with the two regression rows) against mean + dense layers in float64, the bar of
    test_drow_heads_match_mean_and_linears; float16 storage equals the float32 call on the same values; 7 refused."""
    from planar_optical_flow_amd import _lib
    S, C, L = 37, 128, 7
    g = torch.Generator(device=DEV).manual_seed(6)
    feat = torch.randn(S, C, L, device=DEV, generator=g).to(dtype)
    wc, bc = torch.randn(7, C, device=DEV, generator=g), torch.randn(7, device=DEV, generator=g)
    wr, br = torch.randn(2, C, device=DEV, generator=g), torch.randn(2, device=DEV, generator=g)
    cls, reg = ops.drow_heads(feat, wc[:6].contiguous(), bc[:6].contiguous(), wr, br)
    m = feat.double().mean(dim=-1)
    assert torch.allclose(cls.double(), m @ wc[:6].double().T + bc[:6].double(), rtol=1e-5, atol=1e-5)
    assert torch.allclose(reg.double(), m @ wr.double().T + br.double(), rtol=1e-5, atol=1e-5)
    if dtype == torch.float16:
        cls32, reg32 = ops.drow_heads(feat.float(), wc[:6].contiguous(), bc[:6].contiguous(), wr, br)
        assert torch.equal(cls, cls32) and torch.equal(reg, reg32)
    oc = torch.full((S, 7), 7.0, device=DEV)
    orr = torch.full((S, 2), 7.0, device=DEV)
    entry = "pof_drow_heads_f16" if dtype == torch.float16 else "pof_drow_heads"
    _refused(lambda: _lib.call(entry, feat.data_ptr(), S, C, L, wc.data_ptr(), bc.data_ptr(), 7, wr.data_ptr(),
                               br.data_ptr(), oc.data_ptr(), orr.data_ptr(), _stream()), oc, orr)


@pytest.mark.gpu
def test_cutout_limit(ops):
    """Windows of T = 16 scans bit-exact against the atan_mode = "cr" oracle; 17 refused."""
    kw = dict(_DR, num_cutout_pts=56)
    sb = synth.make_batch(seed=17, B=1, T=17, N=450)
    tab, phi = ops.phi_table(), R.laser_phi()
    got = ops.cutout(T(sb.scans[:, :16]), tab, **kw)
    assert np.array_equal(got[0].cpu().numpy(), R.cutout(sb.scans[0, :16], phi, atan_mode="cr", **kw))
    for dt in (torch.float32, torch.float16):
        out = torch.full((1, 450, 17, 56), 7.0, dtype=dt, device=DEV)
        _refused(lambda: ops.cutout(T(sb.scans), tab, out=out, out_dtype=dt, **kw), out)


@pytest.mark.gpu
def test_band_correlation_limit(ops):
    """Kernel 5 with displacement 7 exact against the oracle on integers; kernel 7, displacement 8 and the even kernel
    4 refused, float32 and float16 features."""
    gen = torch.Generator(device="cpu").manual_seed(57)
    for n in (70, 57):                                          # the tiled form and the one-wave form
        f1 = torch.randint(-4, 5, (2, 5, n), generator=gen).float().to(DEV)
        f2 = torch.randint(-4, 5, (2, 5, n), generator=gen).float().to(DEV)
        want = R.band_correlation(f1.double().cpu().numpy(), f2.double().cpu().numpy(), 5, 7).astype(np.float32)
        assert np.array_equal(ops.band_correlation(f1, f2, 5, 7).cpu().numpy(), want)
        assert np.array_equal(ops.band_correlation(f1.half(), f2.half(), 5, 7).cpu().numpy(), want)
        for K, md in ((7, 7), (5, 8), (4, 5)):
            out = torch.full((2, 2 * md + 1, n), 7.0, device=DEV)
            _refused(lambda: ops.band_correlation(f1, f2, K, md, out=out), out)
            _refused(lambda: ops.band_correlation(f1.half(), f2.half(), K, md, out=out), out)
            gout = torch.zeros((2, 2 * md + 1, n), device=DEV)
            _refused(lambda: ops.band_correlation_backward(f1, f2, gout, K, md))


@pytest.mark.gpu
def test_spatial_attention_limit(ops):
    """Window 15 against the oracle at the bars of test_spatial_attention_at_offsets; window 17 and a feature size
    that is no multiple of 4 refused."""
    rng = np.random.default_rng(15)
    B, N, E, F, alpha = 2, 40, 16, 8, 0.4
    ex = T(rng.normal(0, 0.4, (B, N, E)).astype(np.float32))
    et = T(rng.normal(0, 0.4, (B, N, E)).astype(np.float32))
    x = T(rng.normal(0, 1, (B, N, F)).astype(np.float32))
    t = T(rng.normal(0, 1, (B, N, F)).astype(np.float32))
    wo, wb = R.spatial_attention(*(a.double().cpu().numpy() for a in (ex, et, x, t)), alpha, 15)
    out, band, prob = ops.spatial_attention(ex, et, x, t, alpha, 15)
    assert band.shape[-1] == 15
    np.testing.assert_allclose(band.cpu().numpy(), wb, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(out.cpu().numpy(), wo, rtol=1e-4, atol=1e-5)
    for xs, ts in ((x, t), (x.half(), t.half())):
        buf = torch.full((B, N, F), 7.0, dtype=xs.dtype, device=DEV)
        _refused(lambda: ops.spatial_attention(ex, et, xs, ts, alpha, 17, out=buf), buf)
        buf6 = torch.full((B, N, 6), 7.0, dtype=xs.dtype, device=DEV)
        _refused(lambda: ops.spatial_attention(ex, et, xs[..., :6].contiguous(), ts[..., :6].contiguous(), alpha, 15,
                                               out=buf6), buf6)


# ---------------------------------------------------------------- 5. odometry association on an empty range
def _one_sequence(n_odom):
    S = 6
    sb = synth.make_batch(seed=5, B=S, T=1)
    return {"scans": sb.scans[:, 0], "scans_ns": np.arange(S), "scans_t": np.arange(S, dtype=np.float32),
            "odoms_t": np.arange(n_odom, dtype=np.float32), "odoms": np.zeros((n_odom, 3), np.float32),
            "dets_ns": np.arange(0, S, 2), "dets_wc": [[] for _ in range(3)], "dets_wa": [[] for _ in range(3)],
            "dets_wp": [[[2.0, 0.1]] for _ in range(3)], "name": "no_odometry"}


def test_scan_store_refuses_a_sequence_without_odometry(monkeypatch):
    """Scans and zero odometry rows with drop_static=False used to reach associate_odometry_kernel with an empty
    range; the reference fails on it (np.argmin of an empty array).  Refused before anything touches the device."""
    from planar_optical_flow_amd import _lib, scan_store

    def no_launch(*a, **k):
        raise AssertionError("the constructor reached the library")
    monkeypatch.setattr(_lib, "call", no_launch)
    monkeypatch.setattr(scan_store, "DROWBatchPreprocessor", no_launch)
    with pytest.raises(ValueError, match="no_odometry"):
        scan_store.DROWDeviceDataset([_one_sequence(0)], cutout_kwargs=None, drop_static=False)
    with pytest.raises(ValueError, match="argmin"):
        R.associate_odometry(np.zeros(0, np.float32), np.arange(6, dtype=np.float32), 3, [2])


@pytest.mark.gpu
def test_associate_odometry_empty_range(ops):
    """Five samples, the middle one with odom_lo == odom_hi: NaN odometry and index -1 for it (nothing is read), the
    other four equal the oracle, also with a range that starts inside the table."""
    rng = np.random.default_rng(12)
    S, O = 30, 40
    t_s = np.sort(rng.uniform(0, 10, S)).astype(np.float32)
    t_o = np.sort(rng.uniform(0, 10, O)).astype(np.float32)
    odoms = rng.uniform(-5, 5, (O, 3)).astype(np.float32)
    cur = np.array([4, 29, 11, 0, 17], np.int32)
    prev = np.array([3, 25, 10, 0, 12], np.int32)
    lo = np.array([0, 0, 7, 13, 0], np.int32)
    hi = np.array([O, O, 7, O, 21], np.int32)
    od0, od1, i0, i1 = ops.associate_odometry(T(t_s), T(t_o), T(odoms), T(lo), T(hi), T(cur), T(prev))
    od0, od1, i0, i1 = (a.cpu().numpy() for a in (od0, od1, i0, i1))
    for k in range(5):
        if lo[k] == hi[k]:
            assert np.isnan(od0[k]).all() and np.isnan(od1[k]).all() and i0[k] == -1 and i1[k] == -1
            continue
        w0, w1 = R.associate_odometry(t_o[lo[k]:hi[k]], t_s, int(cur[k]), [int(prev[k])])
        assert (int(i0[k]), int(i1[k])) == (w0, w1), k
        assert np.array_equal(od0[k], odoms[lo[k] + w0].astype(np.float64)), k
        assert np.array_equal(od1[k], odoms[lo[k] + w1].astype(np.float64)), k
