"""The split ("sync") form of the fused BatchNorm(train) + LeakyReLU [+ pool] tail at kernel level: one process, no
process group -- the all-reduce between the halves is a torch add of the shards' exchange buffers.

  stats per shard -> add `stat` -> apply per shard;  reduce per shard -> add `red` -> apply per shard
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

# (S, C, L, pool, groups)
SHAPES = [
    (37, 64, 48, 0, 1),       # baseline, no pool
    (37, 128, 48, 1, 1),      # pair pooling
    (6, 6, 10, 1, 1),         # P = 60 is less than one slice; 2 sequences per part
    (300, 64, 48, 1, 1),      # more chunk partials than the 256 threads that sum them
    (12, 16, 256, 0, 2),      # two statistics groups
    (6, 1024, 64, 2, 1),      # row max
    (24, 512, 1, 0, 1),       # dense form: [B, C] seen as L = 1
]
MOMENTUM, EPS, SLOPE = 0.1, 1e-5, 0.1


def _parts(sg):
    """Uneven split of the sg sequences of one statistics group."""
    return {37: (5, 31, 1), 6: (3, 2, 1), 300: (113, 187), 24: (7, 17)}[sg]


def _out_shape(S, C, L, pool):
    return (S, C) if pool == 2 else (S, C, L // 2 if pool else L)


@functools.lru_cache(maxsize=None)
def _case(S, C, L, pool, groups):
    """Inputs of one shape and the float64 torch result on the whole batch (computed once, shared, never modified)."""
    g = torch.Generator(device="cuda").manual_seed(S * 1000 + C + L + pool)
    y = torch.randn(S, C, L, device="cuda", generator=g) * 1.7 + 0.4
    gam = torch.rand(C, device="cuda", generator=g) + 0.5
    bet = torch.randn(C, device="cuda", generator=g) * 0.2
    rm = torch.rand(C, device="cuda", generator=g) * 2 - 1
    rv = torch.rand(C, device="cuda", generator=g) * 1.5 + 0.5
    dz = torch.randn(_out_shape(S, C, L, pool), device="cuda", generator=g)
    y64 = y.double().requires_grad_(True)
    g64, b64 = gam.double().requires_grad_(True), bet.double().requires_grad_(True)
    rm64, rv64 = rm.double().clone(), rv.double().clone()
    outs = []
    for part in y64.chunk(groups, dim=0):
        u = torch.nn.functional.leaky_relu(
            torch.nn.functional.batch_norm(part, rm64, rv64, g64, b64, True, MOMENTUM, EPS), SLOPE)
        outs.append(torch.max(u, 2)[0] if pool == 2 else torch.max_pool1d(u, 2) if pool == 1 else u)
    z64 = torch.cat(outs, dim=0)
    z64.backward(dz.double())
    ref = dict(z=z64.detach(), rm=rm64, rv=rv64, dy=y64.grad, dgam=g64.grad, dbet=b64.grad)
    return dict(y=y, gam=gam, bet=bet, rm=rm, rv=rv, dz=dz), ref


def _shard_rows(S, groups, k):
    """Row indices of shard k: part k of every statistics group, the groups in order."""
    sg = S // groups
    parts = _parts(sg)
    lo = sum(parts[:k])
    return torch.cat([torch.arange(gi * sg + lo, gi * sg + lo + parts[k]) for gi in range(groups)]).cuda()


@pytest.mark.parametrize("S,C,L,pool,groups", SHAPES)
def test_one_shard_untouched_buffers_reproduce_the_one_shot_tail_bit_for_bit(S, C, L, pool, groups):
    """One shard = the whole batch, `stat` and `red` handed on as written: out, save_mean, save_invstd, the running
    statistics, dy, dgamma, dbeta and dbias_in have the bits of bn_lrelu_pool_forward / _backward."""
    from planar_optical_flow_amd import ops
    inp, _ = _case(S, C, L, pool, groups)
    y, gam, bet, dz = inp["y"], inp["gam"], inp["bet"], inp["dz"]
    rm1, rv1, rm2, rv2 = inp["rm"].clone(), inp["rv"].clone(), inp["rm"].clone(), inp["rv"].clone()
    z1, mu1, is1 = ops.bn_lrelu_pool_forward(y, gam, bet, rm1, rv1, MOMENTUM, EPS, SLOPE, pool, groups=groups)
    dy1, dg1, db1, ds1 = ops.bn_lrelu_pool_backward(y, dz, gam, bet, mu1, is1, SLOPE, pool, bias_grad=True,
                                                    groups=groups)
    stat = ops.bn_sync_forward_stats(y, groups=groups)
    z2, mu2, is2 = ops.bn_sync_forward_apply(y, stat, gam, bet, rm2, rv2, MOMENTUM, EPS, SLOPE, pool, groups=groups)
    red, dg2, db2 = ops.bn_sync_backward_reduce(y, dz, gam, bet, mu2, is2, SLOPE, pool, groups=groups)
    dy2, ds2 = ops.bn_sync_backward_apply(y, dz, gam, bet, mu2, is2, red, stat, SLOPE, pool, bias_grad=True,
                                          groups=groups)
    for name, a, b in (("out", z1, z2), ("save_mean", mu1, mu2), ("save_invstd", is1, is2), ("running_mean", rm1, rm2),
                       ("running_var", rv1, rv2), ("dy", dy1, dy2), ("dgamma", dg1, dg2), ("dbeta", db1, db2),
                       ("dbias_in", ds1, ds2)):
        assert a.shape == b.shape and torch.equal(a, b), name
    assert stat.shape == (groups * (2 * C + 1),) and red.shape == (groups * 2 * C,)
    # without the bias sum: the same dy
    assert torch.equal(ops.bn_sync_backward_apply(y, dz, gam, bet, mu2, is2, red, stat, SLOPE, pool, groups=groups), dy1)


@pytest.mark.parametrize("S,C,L,pool,groups", SHAPES)
def test_uneven_shards_match_float64_torch_on_the_whole_batch(S, C, L, pool, groups):
    """The sequences of every group split into uneven parts (one shard = part k of every group): the concatenated
    result against float64 batch_norm(training=True) -> leaky_relu -> pool on the whole batch, at the bars of the
    one-shot tail's tests; the counts add up exactly and every shard reports the same statistics bits."""
    from planar_optical_flow_amd import ops
    inp, ref = _case(S, C, L, pool, groups)
    gam, bet = inp["gam"], inp["bet"]
    sg = S // groups
    rows = [_shard_rows(S, groups, k) for k in range(len(_parts(sg)))]
    assert sorted(torch.cat(rows).tolist()) == list(range(S))
    ys = [inp["y"][r].contiguous() for r in rows]
    dzs = [inp["dz"][r].contiguous() for r in rows]

    stats = [ops.bn_sync_forward_stats(yk, groups=groups) for yk in ys]
    for st, r in zip(stats, rows):      # each shard's own count, written by the kernel
        assert st.view(groups, 2 * C + 1)[:, 2 * C].tolist() == [float(len(r) // groups * L)] * groups
    stat = torch.stack(stats).sum(dim=0)
    assert stat.view(groups, 2 * C + 1)[:, 2 * C].tolist() == [float(sg * L)] * groups       # exactly

    z = torch.empty(_out_shape(S, C, L, pool), device="cuda")
    fwd = []
    for yk, r in zip(ys, rows):
        rm, rv = inp["rm"].clone(), inp["rv"].clone()
        zk, mu, istd = ops.bn_sync_forward_apply(yk, stat, gam, bet, rm, rv, MOMENTUM, EPS, SLOPE, pool, groups=groups)
        z[r] = zk
        fwd.append((mu, istd, rm, rv))
    for mu, istd, rm, rv in fwd[1:]:    # the same global buffer on every shard: the same bits
        assert torch.equal(mu, fwd[0][0]) and torch.equal(istd, fwd[0][1])
        assert torch.equal(rm, fwd[0][2]) and torch.equal(rv, fwd[0][3])
    mu, istd, rm, rv = fwd[0]
    assert torch.allclose(z.double(), ref["z"], rtol=1e-5, atol=2e-5)
    assert torch.allclose(rm.double(), ref["rm"], rtol=1e-5, atol=1e-6)
    assert torch.allclose(rv.double(), ref["rv"], rtol=1e-5, atol=1e-6)

    back = [ops.bn_sync_backward_reduce(yk, dzk, gam, bet, mu, istd, SLOPE, pool, groups=groups)
            for yk, dzk in zip(ys, dzs)]
    red = torch.stack([b[0] for b in back]).sum(dim=0)
    dgam = torch.stack([b[1] for b in back]).double().sum(dim=0)
    dbet = torch.stack([b[2] for b in back]).double().sum(dim=0)
    dy = torch.empty(S, C, L, device="cuda")
    for yk, dzk, r in zip(ys, dzs, rows):
        dy[r] = ops.bn_sync_backward_apply(yk, dzk, gam, bet, mu, istd, red, stat, SLOPE, pool, groups=groups)
    for name, got, want in (("dy", dy.double(), ref["dy"]), ("dgamma", dgam, ref["dgam"]), ("dbeta", dbet, ref["dbet"])):
        err, scale = float((got - want).abs().max()), max(float(want.abs().max()), 1.0)
        assert err <= 1e-4 * scale, (name, err, scale)


def test_sync_tail_rejects_bad_buffers():
    from planar_optical_flow_amd import ops
    y = torch.zeros(4, 8, 8, device="cuda")
    one, zero = torch.ones(8, device="cuda"), torch.zeros(8, device="cuda")
    stat = ops.bn_sync_forward_stats(y)
    with pytest.raises(ValueError):
        ops.bn_sync_forward_apply(y, stat[:-1].contiguous(), one, zero)
    with pytest.raises(TypeError):
        ops.bn_sync_forward_apply(y, stat.float(), one, zero)
    with pytest.raises(ValueError):
        ops.bn_sync_forward_stats(torch.zeros(4, 3, 5, device="cuda"))        # C*L % 4 != 0
    with pytest.raises(TypeError):
        ops.bn_sync_forward_stats(torch.zeros(4, 8, 8))                       # CPU tensor: no fallback
