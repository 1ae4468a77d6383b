"""The backend contract of tvretrieval_amd.inference / tvretrieval_amd.dist (stated at the top of inference.py): the CPU
stand-in of the gloo tests has the names the drivers call, under the parameter names tvretrieval_amd.ops gives them.  This
is the check that replaces probing the backend at run time."""
import inspect

from cpu_backend import CpuOps
from tvretrieval_amd import ops as hip_ops
from tvretrieval_amd.inference import OPS_CONTRACT


def _public_functions(obj):
    return {n: f for n, f in vars(obj).items() if not n.startswith("_") and isinstance(f, staticmethod)}


def test_cpu_ops_functions_exist_in_ops_with_the_same_parameter_names():
    funcs = _public_functions(CpuOps)
    assert funcs
    for name in funcs:
        want = getattr(hip_ops, name, None)
        assert inspect.isfunction(want), "tvretrieval_amd.ops has no function %s" % name
        got_p, want_p = inspect.signature(getattr(CpuOps, name)).parameters, inspect.signature(want).parameters
        assert set(got_p) <= set(want_p), (name, sorted(set(got_p) - set(want_p)))
        for p in got_p:       # a keyword the drivers leave out means the same thing on both sides
            if want_p[p].default is not inspect.Parameter.empty and got_p[p].default is not inspect.Parameter.empty:
                assert got_p[p].default == want_p[p].default, (name, p)


def test_every_contract_name_exists_on_both_backends():
    assert len(set(OPS_CONTRACT)) == len(OPS_CONTRACT)
    for name in OPS_CONTRACT:
        assert hasattr(hip_ops, name), name
        assert hasattr(CpuOps, name), name
    callables = {n for n in OPS_CONTRACT if callable(getattr(hip_ops, n)) and n != "F16S"}
    assert callables <= set(_public_functions(CpuOps))
