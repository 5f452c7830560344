"""Host-only launch plans (no GPU needed): the kernel form the conv trunk launcher picks and the segment lengths of the
spatial attention walks, from the size of a launch.  The launchers call the same host functions, so these answers
are what runs.  Checked here: the forms production shapes run, and that the parameter tables of
tests/test_launch_size_gpu.py (tests/cases.py) launch every form the selection rules can produce."""
import pytest

import cases


@pytest.fixture(scope="module")
def ops():
    from planar_optical_flow_amd import build, _lib
    build.build(verbose=False)
    _lib.load()
    from planar_optical_flow_amd import ops as _ops
    return _ops


def _form(ops, S, Ci, Co, L, kernel=3, stride=1, pool=False, fused=False):
    p = ops.conv1d_plan(S, Ci, Co, L, kernel, stride, pool, fused)
    return ("splitk" if p["split_k"] else "ct") + str(p["channels_per_workgroup"]) + \
        ("q" if cases.conv_quantised(S, Co, L, stride, p) else "")


def test_production_shapes(ops):
    """DR-SPAAM (S = windows x 5 scans x 450 cutouts through blocks 1-2, windows x 450 through blocks 3-4) and the
    Prototype at the README's batches run the 128-channel and quantised 64-channel tiles; streaming runs split K;
    attention at production batches walks segments of 29 .. 450 points."""
    f = lambda *a, **k: _form(ops, *a, **k)
    # DR-SPAAM forward at 32 windows (README row)
    S12, S34 = 32 * 5 * 450, 32 * 450
    assert f(S12, 64, 64, 56, fused=True) == "ct64"
    for Ci, Co, L in ((64, 128, 56), (128, 128, 28), (128, 256, 28)):
        assert f(S12, Ci, Co, L) == "ct128", (Ci, Co, L)
    for Ci, Co in ((256, 256), (256, 512)):
        assert f(S34, Ci, Co, 14) == "ct128", (Ci, Co)
    for Ci, Co in ((512, 256), (256, 128)):
        assert f(S34, Ci, Co, 7) == "ct64q", (Ci, Co)
    # training batch: 8 windows, cutouts of 56 or 48 points
    for P in (56, 48):
        S12, S34 = 8 * 5 * 450, 8 * 450
        for Ci, Co, L in ((64, 128, P), (128, 128, P // 2), (128, 256, P // 2)):
            assert f(S12, Ci, Co, L) == "ct128", (P, Ci, Co, L)
        for Ci, Co in ((256, 256), (256, 512)):
            assert f(S34, Ci, Co, P // 4) == "ct64q", (P, Ci, Co)
    # streaming: one window, one scan through every block
    S = 450
    assert f(S, 64, 128, 56) == "ct64"
    assert f(S, 128, 128, 28) == "splitk32"
    assert f(S, 256, 256, 14) == "splitk32"
    assert f(S, 512, 256, 7) == "splitk64"
    # Prototype at 4096 pairs: both scans through the stride-2 encoders, the pairs through the decoders
    assert f(8192, 1, 64, 450, stride=2) == "ct64"
    assert f(8192, 64, 128, 225, stride=2) == "ct128"
    assert f(8192, 128, 256, 113, stride=2) == "ct128"
    assert f(4096, 139, 128, 57) == "ct64q"
    assert f(4096, 192, 128, 113) == "ct128"
    assert f(4096, 129, 2, 450, kernel=1) == "ct32"            # the one point-wise unit has two output channels
    # attention: (forward merge, fused backward) segments
    plan = ops.spatial_attention_plan
    assert plan(256, 450, 3584)[0] == 225
    assert plan(64, 450, 3584)[1] == 57
    assert plan(32, 450, 3584) == (29, 29)
    assert plan(439, 450, 3584) == (450, 450) and plan(438, 450, 3584) == (225, 225)
    assert plan(1, 450, 3584) == (8, 15)


def test_plan_counts_launches_and_wide_offsets(ops):
    """Sequences go in chunks of < 2^30 input elements; a launch that writes >= 2^30 output elements is counted."""
    assert ops.conv1d_plan(150000, 512, 32, 14, pool=True)["launches"] == 2
    assert ops.conv1d_plan(160000, 64, 128, 56)["wide_offsets"] == 1
    assert ops.conv1d_plan(140000, 64, 128, 56)["wide_offsets"] == 0
    with pytest.raises(AssertionError):
        ops.conv1d_plan(0, 4, 4, 8)
    with pytest.raises(Exception):
        ops.conv1d_plan(4, 4, 4, 8, kernel_size=1, stride=2)
    with pytest.raises(Exception):
        ops.conv1d_plan(4, 129, 4, 8, fused_first=True)
    with pytest.raises(Exception):
        ops.spatial_attention_plan(1, 450, 3583)


def test_gpu_tables_reach_every_form(ops):
    """The cases of tests/test_launch_size_gpu.py between them launch every conv family x {32, 64, 128} channels,
    split K with 32 and 64 channels, the quantised 64-channel form, ragged Co = 130 / 70 at 128 and 64 channels,
    64-bit output offsets, and attention segments from the shortest (B = 1) to the whole scan."""
    seen = set()
    for case in cases.CONV_FORM_CASES:
        family, Ci, Co, L, pool, cpw, split, quantised = case
        kernel, stride = cases.CONV_FAMILIES[family]
        S = cases.conv_case_batch(ops.conv1d_plan, case)
        p = ops.conv1d_plan(S, Ci, Co, L, kernel, stride, pool, family == "fused")
        assert (p["split_k"], p["channels_per_workgroup"], p["launches"]) == (split, cpw, 1), (case, S, p)
        assert cases.conv_quantised(S, Co, L, stride, p) == quantised, (case, S)
        seen.add((family, "splitk" if split else "ct", cpw))
        if quantised:
            seen.add((family, "quantised"))
        if Co in (70, 130) and not split:
            seen.add(("ragged", Co, cpw))
        if stride == 2 and L % 2:
            seen.add("odd stride-2 L")
        seen.add(("pool", pool))
    want = {(f, "ct", c) for f in cases.CONV_FAMILIES for c in (32, 64, 128)}
    want |= {("k3s1", "splitk", 32), ("k3s1", "splitk", 64), ("k3s1", "quantised")}
    want |= {("ragged", Co, c) for Co in (70, 130) for c in (64, 128)}
    want |= {"odd stride-2 L", ("pool", True), ("pool", False)}
    assert want <= seen, sorted(map(str, want - seen))
    family, Ci, Co, L, pool, S = cases.CONV_WIDE_CASE
    assert ops.conv1d_plan(S, Ci, Co, L, *cases.CONV_FAMILIES[family], pool)["wide_offsets"] >= 1
    fwd, bwd = set(), set()
    for B, N, f, b in cases.ATTENTION_CASES:
        assert ops.spatial_attention_plan(B, N, cases.ATTENTION_F) == (f, b), (B, N)
        single = ops.spatial_attention_plan(1, N, cases.ATTENTION_F)       # the B = 1 launches each case compares with
        fwd |= {f, single[0]}
        bwd |= {b, single[1]}
    assert min(fwd) <= 8 and {29, 57, 225, 450} <= fwd, sorted(fwd)
    # the fused backward's segments stop halving at 16 points
    assert min(bwd) <= 16 and {29, 57, 225, 450} <= bwd, sorted(bwd)
