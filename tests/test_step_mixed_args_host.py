"""BatchEnvironment.step_mixed's argument checks without a GPU, in the manner of tests/test_wrapper_args_host.py: a BatchEnvironment made
with __new__ whose library is a recording stand-in, duck tensors in place of device tensors (tests/wrapper_standin.py).  A refused row
raises a ValueError that names the argument and reaches NO library function; right tensors reach the one entry point,
pom_batch_step_mixed, with the spec's fields as given.  step_mixed makes no runtime call and needs no torch."""
import ctypes as C
from types import SimpleNamespace

import pytest

from pomcpp_amd.batch import BatchEnvironment, _MixedStepSpec
from tests import wrapper_standin as W
from tests.test_wrapper_args_host import _bad
from tests.wrapper_standin import Duck, N

I32, U8, F16 = W.I32, W.U8, W.F16


def _handle():
    return W.handle(BatchEnvironment)


def _spec_of(env):
    (entry, args), = env._lib.calls
    env._lib.calls.clear()
    assert entry == "pom_batch_step_mixed" and len(args) == 2
    spec = args[1]._obj   # (byref's object: the spec the call built)
    assert isinstance(spec, _MixedStepSpec) and spec.struct_size == C.sizeof(_MixedStepSpec) == 104
    assert (spec.flags, spec.reserved_) == (0, 0)
    return spec


def _rows(env):
    """(argument, the name a refusal must carry, element type, shape, how the tensor is passed)"""
    mv = lambda: Duck((N, 4), I32)  # noqa: E731
    views = lambda: Duck((N, 4, 16, 11, 11), U8)  # noqa: E731
    return [
        ("moves", "moves", I32, (N, 4), lambda t: env.step_mixed(0, 16, t, 0b1110, 1, 2)),
        ("codes", "codes", U8, (N, 5, 11, 11), lambda t: env.step_mixed(0, 16, mv(), 0b1110, 1, 2, codes=t)),
        ("planes", "planes", U8, (N, 16, 11, 11), lambda t: env.step_mixed(0, 16, mv(), 0b1110, 1, 2, planes=t)),
        ("planes, per_agent", "planes", U8, (N, 4, 16, 11, 11), lambda t: env.step_mixed(0, 16, mv(), 0b1110, 1, 2, planes=t, per_agent=True)),
        ("agent_attrs", "agent_attrs", I32, (N, 4, 8), lambda t: env.step_mixed(0, 16, mv(), 0b1110, 1, 2, planes=Duck((N, 16, 11, 11), U8), agent_attrs=t)),
        ("env_attrs", "env_attrs", I32, (N, 4), lambda t: env.step_mixed(0, 16, mv(), 0b1110, 1, 2, planes=Duck((N, 16, 11, 11), U8), env_attrs=t)),
        ("codes, view", "codes", U8, (N, 4, 5, 11, 11), lambda t: env.step_mixed(0, 16, mv(), 0b1110, 1, 2, codes=t, view_radius=4)),
        ("planes, view", "planes", U8, (N, 4, 16, 11, 11), lambda t: env.step_mixed(0, 16, mv(), 0b1110, 1, 2, planes=t, view_radius=4)),
        ("viewer_attrs", "viewer_attrs", I32, (N, 4, 12), lambda t: env.step_mixed(0, 16, mv(), 0b1110, 1, 2, planes=views(), view_radius=4, viewer_attrs=t)),
        ("env_attrs, view", "env_attrs", I32, (N, 4), lambda t: env.step_mixed(0, 16, mv(), 0b1110, 1, 2, planes=views(), view_radius=4, env_attrs=t)),
    ]


def test_refused_rows_reach_no_library_function():
    env = _handle()
    wrong, n = [], 0
    for arg, name, dtype, shape, fn in _rows(env):
        for what, t in _bad(dtype, shape):
            n += 1
            try:
                fn(t)
                wrong.append(f"{arg}, {what}: accepted")
            except ValueError as e:
                if name not in str(e):
                    wrong.append(f"{arg}, {what}: the text does not name {name!r}: {e}")
            if env._lib.calls:
                wrong.append(f"{arg}, {what}: reached {env._lib.calls[0][0]}")
                env._lib.calls.clear()
    assert n == 80 and not wrong, f"{len(wrong)} of {n} rows:\n" + "\n".join(wrong)


def test_right_tensors_reach_the_one_entry_point_with_the_specs_fields_as_given():
    env = _handle()
    for arg, name, dtype, shape, fn in _rows(env):
        t = Duck(shape, dtype)
        fn(t)
        spec = _spec_of(env)
        assert (spec.simple_mask, spec.first, spec.count, spec.seed, spec.tick, spec.stream) == (0b1110, 0, 16, 1, 2, None), arg
        if "view" in arg:
            assert spec.view and (spec.planes_dev, spec.agent_attrs_dev, spec.env_attrs_dev) == (None, None, None), arg
            v = spec.view.contents
            assert v.struct_size == C.sizeof(v) and v.view_radius == 4 and v.dtype == (3 if "codes" in arg else 0), arg
            got = (spec.moves_dev, v.planes_dev, v.viewer_attrs_dev, v.env_attrs_dev)
        else:
            assert not spec.view, arg
            got = (spec.moves_dev, spec.planes_dev, spec.agent_attrs_dev, spec.env_attrs_dev)
            if arg != "moves":
                assert (spec.dtype, spec.per_agent) == (3 if arg == "codes" else 0, int("per_agent" in arg)), arg
        assert [g for g in got if g == t.address] == [t.address], arg


def test_every_field_as_given():
    env = _handle()
    mv, planes = Duck((N, 4), I32), Duck((N, 4, 16, 11, 11), F16)
    a, e = Duck((N, 4, 8), I32), Duck((N, 4), I32)
    env.step_mixed(16, 4, mv, [1, 3], (1 << 64) + 5, 0xFFFFFFFF, SimpleNamespace(cuda_stream=0x77), planes=planes, per_agent=True, agent_attrs=a, env_attrs=e)
    s = _spec_of(env)
    assert (s.simple_mask, s.first, s.count, s.moves_dev, s.seed, s.tick, s.stream) == (0b1010, 16, 4, mv.address, 5, 0xFFFFFFFF, 0x77)
    assert (s.planes_dev, s.dtype, s.per_agent, s.agent_attrs_dev, s.env_attrs_dev) == (planes.address, 1, 1, a.address, e.address) and not s.view
    env.step_mixed(0, N, None, 0xF, 7, 0)   # all four agents: no moves, no observation
    s = _spec_of(env)
    assert (s.simple_mask, s.moves_dev, s.planes_dev, s.dtype, s.per_agent) == (15, None, None, 0, 0) and not s.view
    env.step_mixed(0, 0, 0x1000, 0, 7, 3, 0x99, 0x2000)   # raw addresses pass unchecked (codes then)
    s = _spec_of(env)
    assert (s.simple_mask, s.count, s.moves_dev, s.stream, s.planes_dev, s.dtype) == (0, 0, 0x1000, 0x99, 0x2000, 3)


def test_contradictions_masks_ticks_and_ranges_are_refused():
    env = _handle()
    mv, codes, planes = Duck((N, 4), I32), Duck((N, 5, 11, 11), U8), Duck((N, 16, 11, 11), U8)
    attrs = Duck((N, 4, 8), I32)
    for kw in (dict(codes=codes, planes=planes), dict(codes=codes, per_agent=True), dict(agent_attrs=attrs), dict(per_agent=True),
               dict(env_attrs=Duck((N, 4), I32)), dict(planes=planes, viewer_attrs=Duck((N, 4, 12), I32)),
               dict(planes=Duck((N, 4, 16, 11, 11), U8), view_radius=4, agent_attrs=attrs), dict(view_radius=4),
               dict(planes=Duck((N, 4, 16, 11, 11), U8), view_radius=11)):
        with pytest.raises(ValueError):
            env.step_mixed(0, 16, mv, 0b1110, 1, 2, **kw)
    for first, count in ((-16, 16), (0, N + 1), (16, N), (N, 1), (0, -1)):
        with pytest.raises(ValueError, match="outside the batch"):
            env.step_mixed(first, count, mv, 0b1110, 1, 2)
    for simple in (16, -1, [4], 1.5, True):
        with pytest.raises(ValueError, match="simple"):
            env.step_mixed(0, 16, mv, simple, 1, 2)
    for tick in (-1, 1 << 32):
        with pytest.raises(ValueError, match="tick"):
            env.step_mixed(0, 16, mv, 0b1110, 1, tick)
    for simple in (0, 0b0111, [0, 1]):
        with pytest.raises(ValueError, match="moves"):
            env.step_mixed(0, 16, None, simple, 1, 2)
    assert not env._lib.calls
