"""The scenes of tests/test_icp_rules.py on the GPU: every rule of the ICP core (csrc/pof_icp.h) and of the keyframe
policies taken at equality, through ops.scan_match, ops.keyframe_match and ops.keyframe_map_match, in both kernel forms
(one wave for N <= 512, 512 threads with the slot layout t + 512 c above) and at the three placements, against the
float64 restatements.  The cases of one entry point and one scan length that share a table and the settings make one
launch.

Compared as equal values (NaN where NaN; the sign of a zero is not looked at, FMA contraction may choose it): count,
ok, iters_used, corr, key_replaced, key_switched, key_slot, every state field with the stored key_ranges, and motion,
rms, flow_residual, key_rel, pose, key_pose, rot, trans, flow_trans, which the scenes make exact.  With a tolerance:
obs, which passes through the Cholesky factor -- the project's rule (100 x the pairwise-against-sequential disagreement
of the restatement, at least 1e-13), which on exact sums is its floor
(tests/test_icp_rules.test_the_sums_are_exact_so_the_tolerance_rule_gives_its_floor).  No other tolerance."""
import numpy as np
import pytest
import torch

from test_icp_rules import ENTRIES, KEYS, SCENES, TOL, all_cases, case, differences, restatement, want

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from planar_optical_flow_amd import ops as _ops
    return _ops


def _cuda(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def launches(keys):
    """The cases `keys` grouped into launches: same entry point, length, table and settings."""
    groups = {}
    for key in keys:
        c = case(*key)
        groups.setdefault((c["entry"], c["N"], c["tab"].tobytes(), tuple(sorted(c["settings"].items()))), []).append(key)
    return list(groups.values())


class Launch:
    """One launch of the cases `keys` in fixed buffers: prime() loads the state, run() launches, host() -> per sensor
    (state after or None, outputs) as the restatement returns them."""

    def __init__(self, ops, keys, repeat=1):
        self.ops, self.keys = ops, [k for k in keys for _ in range(repeat)]
        self.cases = [case(*k) for k in self.keys]
        c = self.cases[0]
        self.entry, self.N, self.B, self.kw = c["entry"], c["N"], len(self.cases), c["settings"]
        self.tab = _cuda(c["tab"], np.float64)
        self.cur = _cuda(np.stack([c["r1"] for c in self.cases]), np.float32)
        if self.entry == "scan_match":
            self.prev = _cuda(np.stack([c["r0"] for c in self.cases]), np.float32)
            inits = [c["init"] for c in self.cases]
            self.init = None if all(i is None for i in inits) else \
                _cuda(np.stack([np.zeros(3) if i is None else i for i in inits]), np.float64)
            self.out = ops.scan_match_buffers(self.B, self.N)
            return
        self.terms = dict(rot=torch.zeros(self.B, 4, device="cuda"),
                          trans=torch.zeros(self.B, 2, dtype=torch.float64, device="cuda"),
                          flow_trans=torch.zeros(self.B, 2, dtype=torch.float64, device="cuda"))
        if self.entry == "keyframe":
            self.state, self.out = ops.keyframe_buffers(self.B, self.N), ops.keyframe_match_buffers(self.B, self.N)
        else:
            self.state = ops.keyframe_map_buffers(self.B, self.N, KEYS)
            self.out = ops.keyframe_map_match_buffers(self.B, self.N)
        self.primed = {k: _cuda(np.stack([np.asarray(c["state"][k]) for c in self.cases])) for k in self.state._fields}
        for k in self.state._fields:
            assert self.primed[k].dtype == getattr(self.state, k).dtype and self.primed[k].shape == getattr(self.state, k).shape, k

    def prime(self):
        if self.entry != "scan_match":
            for k in self.state._fields:
                getattr(self.state, k).copy_(self.primed[k])

    def run(self, out=None, init="own"):
        out = self.out if out is None else out
        if self.entry == "scan_match":
            self.ops.scan_match(self.prev, self.cur, self.tab, init=self.init if init == "own" else init, out=out, **self.kw)
        elif self.entry == "keyframe":
            self.ops.keyframe_match(self.cur, self.tab, self.state, out=out, **self.terms, **self.kw)
        else:
            self.ops.keyframe_map_match(self.cur, self.tab, self.state, out=out, **self.terms, **self.kw)

    def host(self, out=None):
        out = self.out if out is None else out
        o = {k: getattr(out, k).cpu().numpy() for k in out._fields}
        s = None
        if self.entry != "scan_match":
            o.update({k: v.cpu().numpy() for k, v in self.terms.items()})
            s = {k: getattr(self.state, k).cpu().numpy() for k in self.state._fields}
        return [(None if s is None else {k: v[b] for k, v in s.items()}, {k: v[b] for k, v in o.items()})
                for b in range(self.B)]

    def step(self):
        self.prime()
        self.run()
        return self.host()


def _check(got, key):
    ref = want(key)
    assert set(ref[1]) - {"margins"} <= set(got[1]) and (ref[0] is None or set(ref[0]) == set(got[0])), key
    wrong = differences(got, ref, tol=TOL)
    assert wrong == {}, (key, SCENES[key[0]]["rule"], wrong, {k: (got[1].get(k), ref[1].get(k)) for k in wrong if k in ref[1]})


# ------------------------------------------------------------------ 1. every scene, entry point, form and placement
@pytest.mark.parametrize("N", ["own", 512, 513, 4096])
@pytest.mark.parametrize("entry", ENTRIES)
def test_device_takes_every_rule_as_the_restatement_does(ops, entry, N):
    keys = [k for k in all_cases(entry) if k[2] == N]
    groups = launches(keys)
    for group in groups:
        for got, key in zip(Launch(ops, group).step(), group):
            _check(got, key)
    rules = {SCENES[k[0]]["rule"] for k in keys} - {None}
    print("%s N=%s: %d cases in %d launches (largest %d sensors), %d rules at equality, placements %s"
          % (entry, N, len(keys), len(groups), max(len(g) for g in groups), len(rules), sorted({k[3] for k in keys})))
    assert len(rules) >= 12 and len(keys) >= 30


# ------------------------------------------------------------------ 2. the start value in the motion buffer
@pytest.mark.parametrize("N", ["own", 4096])
def test_init_may_be_the_motion_buffer_of_the_same_call(ops, N):
    key = ("alias", "scan_match", N, "own" if N == "own" else "wrap")
    launch = Launch(ops, [key], repeat=3)
    out = ops.scan_match_buffers(3, launch.N)
    out.motion.copy_(launch.init)
    launch.run(out=out, init=out.motion)
    for got in launch.host(out):
        _check(got, key)
        assert got[1]["ok"] and np.array_equal(got[1]["motion"], [0.0, 0.25, 0.0])


# ------------------------------------------------------------------ 3. one slot is pof_keyframe_match
def test_one_slot_has_the_bits_of_keyframe_match_on_the_rule_scenes(ops):
    n = 0
    for group in launches([k for k in all_cases("keyframe") if k[2] in ("own", 513)]):
        single = Launch(ops, group)
        got = single.step()
        B, N = single.B, single.N
        ring, out = ops.keyframe_map_buffers(B, N, 1), ops.keyframe_map_match_buffers(B, N)
        terms = {k: torch.zeros_like(v) for k, v in single.terms.items()}
        for k in single.state._fields:
            getattr(ring, k).copy_(single.primed[k].reshape(getattr(ring, k).shape))
        ops.keyframe_map_match(single.cur, single.tab, ring, out=out, **terms, **dict(single.kw, revisit=0.5))
        for b in range(B):
            for k, v in got[b][1].items():
                other = terms[k] if k in terms else getattr(out, k)
                assert np.array_equal(other[b].cpu().numpy(), v, equal_nan=True), (group[b], k)
            for k, v in got[b][0].items():
                assert np.array_equal(getattr(ring, k)[b].cpu().numpy().reshape(v.shape), v, equal_nan=True), (group[b], k)
        assert not out.key_switched.any() and not out.key_slot.any()
        n += B
    assert n >= 60


# ------------------------------------------------------------------ 4. the same bits anywhere, again and in a graph
def _same(a, b, what):
    for x, y in zip(a, b):
        for k in x or {}:
            assert np.array_equal(x[k], y[k], equal_nan=True), (what, k)


@pytest.mark.parametrize("entry,N,where", [("scan_match", 512, "end"), ("keyframe_map", 4096, "wrap")])
def test_the_same_bits_at_five_batch_positions_in_two_runs_and_in_a_graph(ops, entry, N, where):
    """One family per kernel form: the tie, gate and corner scenes (N8, one wave) and the ring scenes with window = 64
    (N10, 512 threads)."""
    names = ("tie_mid", "gate_eq", "corner") if entry == "scan_match" else ("rev_eq", "rev_two", "lru")
    for name in names:
        key = (name, entry, N, where)
        launch = Launch(ops, [key], repeat=5)
        if entry == "keyframe_map":
            launch.kw = dict(launch.kw, window=64)              # the widest window; the scene's vertices stay inside
        first, second = launch.step(), launch.step()
        for b in range(5):
            for half in (0, 1):
                _same([first[0][half]], [first[b][half]], (key, b))
                _same([first[0][half]], [second[b][half]], (key, b, "again"))
        ref = restatement(launch.cases[0], window=launch.kw["window"])
        assert differences(first[0], ref, tol=TOL) == {}, (key, differences(first[0], ref, tol=TOL))
        # the same call captured and replayed twice
        captured = type(launch.out)(*(torch.zeros_like(t) for t in launch.out))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            launch.prime()
            launch.run(out=type(launch.out)(*(torch.zeros_like(t) for t in launch.out)))     # warm-up
        torch.cuda.current_stream().wait_stream(side)
        launch.prime()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            launch.run(out=captured)
        for _ in range(2):
            for t in captured:
                t.zero_()
            launch.prime()
            graph.replay()
            again = launch.host(captured)
            for b in range(5):
                _same([first[b][1]], [again[b][1]], (key, b, "graph"))
                _same([first[b][0]], [again[b][0]], (key, b, "graph state"))
