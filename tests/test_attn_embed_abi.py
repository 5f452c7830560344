"""Host-only: the gate-embedding entry points are declared in include/pof_abi.h, exported by the library
and bound by _lib; the model's ``embed`` option validates and resets; the plan query answers without a device."""
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declaration(text, name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, "include/pof_abi.h does not declare %s" % name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_attn_embed_entries_declared_exported_and_bound():
    from planar_optical_flow_amd import build, _lib
    build.build(verbose=False)
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "pof_abi.h")).read(), flags=re.S)
    args, twin_args = _declaration(text, "pof_attn_embed_f16"), _declaration(text, "pof_attn_embed")
    for name in ("pof_attn_embed", "pof_attn_embed_f16"):
        assert hasattr(lib, name), "libpof_hip.so does not export %s" % name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is _lib._i and len(argtypes) == len(args) == len(twin_args) == 11
        # NULL operands are refused before any launch
        assert getattr(lib, name)(*[None if t is _lib._p else 0 for t in argtypes]) == _lib.POF_E_BADARG
    assert list(_lib.SIGNATURES["pof_attn_embed_f16"][1]) == list(_lib.SIGNATURES["pof_attn_embed"][1])
    for a, t in zip(args, twin_args):
        # the two row operands become `const void *..._f16`; every other parameter is the twin's, word for word
        if a.endswith("_f16"):
            assert re.fullmatch(r"const void \*\w+_f16", a) and t.startswith("const float *")
        else:
            assert a == t, (a, t)
    assert sum(a.endswith("_f16") for a in args) == 2
    assert twin_args[2] == "long long R" and twin_args[7] == "double negative_slope"


def test_plan_is_stable_across_the_ranges_it_documents():
    """form 0 for 1 <= R < 8192, form 1 from 8192 rows on, whatever K and E; bad shapes are refused as the launcher
    refuses them.  No device work."""
    from planar_optical_flow_amd import _lib, ops
    for K, E in ((8, 32), (512, 128), (3584, 128), (3072, 256)):
        assert {ops.attn_embed_plan(R, K, E) for R in (1, 2, 31, 32, 33, 450, 907, 3600, 8191)} == {0}
        assert {ops.attn_embed_plan(R, K, E) for R in (8192, 8193, 14400, 1 << 20, 1 << 33)} == {1}
    for R, K, E in ((1, 12, 128), (1, 8, 48), (1, 8, 288), (1, 8, 16)):
        with pytest.raises(_lib.PofError) as err:
            ops.attn_embed_plan(R, K, E)
        assert err.value.code == _lib.POF_E_SHAPE
    with pytest.raises(AssertionError):
        ops.attn_embed_plan(0, 8, 32)
    assert _lib.load().pof_attn_embed_plan(1, 8, 32, None) == _lib.POF_E_BADARG


def test_embed_option_validates_and_resets():
    import torch
    from planar_optical_flow_amd.src.depracted.model.dr_spaam import DROW, SpatialDROW, _SpatialAttention
    torch.manual_seed(0)
    model = SpatialDROW(num_pts=48, window_size=7).eval()
    with pytest.raises(ValueError):
        model.fuse_for_inference(embed="bogus")
    with pytest.raises(ValueError):
        model.gate.fold_for_inference(embed="bogus")
    with pytest.raises(ValueError):
        DROW(num_pts=48).fuse_for_inference(embed="bogus")
    assert getattr(model, "_fused", None) is None                # a refused call fused nothing
    model.fuse_for_inference()
    assert model._embed_route == model.gate._embed_route == "library"
    model.fuse_for_inference(storage=torch.float16, embed="hip")
    assert model._embed_route == model.gate._embed_route == "hip" and model.gate._storage == torch.float16
    model.fuse_for_inference(False)
    assert model._embed_route == model.gate._embed_route == "library" and model.gate._folded is None
    model.fuse_for_inference(embed="hip")
    model.train()
    assert model._embed_route == model.gate._embed_route == "library"
    assert model._fused is None and model.gate._folded is None
    gate = _SpatialAttention(n_pts=12, n_channel=256).eval()
    gate.fold_for_inference(True, torch.float32, "hip")
    assert gate._embed_route == "hip"
    gate.train()
    assert gate._embed_route == "library"


def test_ops_refuse_cpu_and_bfloat16_rows():
    import torch
    from planar_optical_flow_amd import ops
    w, b = torch.zeros(32, 8), torch.zeros(32)
    with pytest.raises(TypeError):
        ops.attn_embed(torch.zeros(2, 8), None, w, b, 0.1)
    with pytest.raises(TypeError):
        ops.attn_embed(torch.zeros(2, 8, dtype=torch.float16), torch.zeros(2, 8, dtype=torch.float16), w, b, 0.1)
    with pytest.raises(TypeError):
        ops.attn_embed(torch.zeros(2, 8, dtype=torch.bfloat16), None, w, b, 0.1)
