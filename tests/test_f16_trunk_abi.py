"""Host-only: the float16-storage trunk entry points are declared in include/pof_abi.h, exported by the
library and bound by _lib with the arity and argument kinds of their float32 twins."""
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWINS = {"pof_conv3_bn_lrelu_f16": "pof_conv3_bn_lrelu", "pof_conv3_first_two_f16": "pof_conv3_first_two",
         "pof_drow_heads_f16": "pof_drow_heads"}


def _declaration(text, name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, "include/pof_abi.h does not declare %s" % name
    return [a.strip() for a in m.group(1).split(",")]


def test_float16_trunk_entries_declared_exported_and_bound():
    from planar_optical_flow_amd import build, _lib
    build.build(verbose=False)
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "pof_abi.h")).read(), flags=re.S)
    for name, twin in TWINS.items():
        args, twin_args = _declaration(text, name), _declaration(text, twin)
        assert hasattr(lib, name), "libpof_hip.so does not export %s" % name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is _lib._i and len(argtypes) == len(args) == len(twin_args)
        assert list(argtypes) == list(_lib.SIGNATURES[twin][1])
        for a, t in zip(args, twin_args):
            # the activations become `void *..._f16`; every other parameter is the twin's, word for word
            if a.endswith("_f16"):
                assert re.fullmatch(r"(const )?void \*\w+_f16", a) and t.startswith("const float *" if "const" in a else "float *")
            else:
                assert a == t, (name, a, t)
        assert sum(a.endswith("_f16") for a in args) == (1 if name == "pof_drow_heads_f16" else 2)
        # NULL activations are refused before any launch
        assert getattr(lib, name)(*[None if t is _lib._p else 0 for t in argtypes]) == _lib.POF_E_BADARG


def test_ops_refuse_cpu_float16():
    import torch
    from planar_optical_flow_amd import ops
    with pytest.raises(TypeError):
        ops.conv3_bn_lrelu(torch.zeros(2, 1, 56, dtype=torch.float16), torch.zeros(3, 1, 64), torch.ones(64), torch.zeros(64))
    with pytest.raises(TypeError):
        ops.drow_heads(torch.zeros(2, 128, 7, dtype=torch.float16), torch.zeros(1, 128), torch.zeros(1), torch.zeros(2, 128),
                       torch.zeros(2))
