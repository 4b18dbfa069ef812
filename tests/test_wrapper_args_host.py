"""BatchEnvironment's argument checks without a GPU: every row of tests/test_wrapper_args.py's table, driven against a BatchEnvironment
made with __new__ whose library is a recording stand-in, with duck tensors (data_ptr / shape / dtype / is_contiguous / device) in place
of device tensors (tests/wrapper_standin.py).  A refused row raises a ValueError that names the argument and reaches NO library
function — on a real handle it would have launched a kernel on a bad address —; a right tensor reaches exactly the one entry point,
with the addresses, the element type's code and per_agent it should.  step_device_range makes no runtime call, so its tests need no
torch at all; for the calls that allocate their results a stand-in module serves as torch."""
import ctypes as C
import sys

import pytest

from pomcpp_amd.batch import BatchEnvironment, _ViewSpec
from tests import wrapper_standin as W
from tests.test_wrapper_args import N, other_rows, range_rows
from tests.wrapper_standin import Duck

I8, I32, I64, U8 = W.I8, W.I32, W.I64, W.U8


def _handle():
    return W.handle(BatchEnvironment)


def _bad(dtype, shape, free=False):
    """tests/test_wrapper_args._bad as ducks: (what is wrong, tensor); a `free` first dimension is the caller's, as there"""
    yield "dtype", Duck(shape, "torch.int64" if dtype == I32 else I32)
    yield "dtype, float for bytes", Duck(shape, "torch.float64")
    yield "shape, one dimension more", Duck(shape + (2,), dtype)
    if not free or len(shape) > 1:
        yield "shape, last dimension", Duck(shape[:-1] + (shape[-1] + 1,), dtype)
    if not free:
        yield "shape, first dimension", Duck((shape[0] + 1,) + shape[1:], dtype)
        yield "shape, the range's instead of the batch's", Duck((16,) + shape[1:], dtype)
    yield "a strided slice", Duck(shape, dtype, contiguous=False)
    yield "on the CPU", Duck(shape, dtype, device="cpu")


def test_refused_rows_reach_no_library_function():
    env = _handle()
    rows = range_rows(env, I32, U8, Duck)
    assert {r[1] for r in rows} == {"moves", "codes", "planes", "agent_attrs", "env_attrs", "viewer_attrs"} and len(rows) == 10
    wrong, n = [], 0
    for call, arg, name, dtype, shape, _, fn in rows:
        for what, t in _bad(dtype, shape):
            n += 1
            try:
                fn(t)
                wrong.append(f"{call} {arg}, {what}: accepted")
            except ValueError as e:
                if name not in str(e):
                    wrong.append(f"{call} {arg}, {what}: the text does not name {name!r}: {e}")
            if env._lib.calls:
                wrong.append(f"{call} {arg}, {what}: reached {env._lib.calls[0][0]}")
                env._lib.calls.clear()
    assert n == 80 and not wrong, f"{len(wrong)} of {n} rows:\n" + "\n".join(wrong)


def test_right_tensors_reach_the_one_entry_point():
    env = _handle()
    for call, arg, name, dtype, shape, _, fn in range_rows(env, I32, U8, Duck):
        t = Duck(shape, dtype)
        fn(t)
        (entry, args), = env._lib.calls
        env._lib.calls.clear()
        assert entry == ("pom_batch_step_device_range_view" if "view" in call else "pom_batch_step_device_range"), call
        assert args[1:3] == (0, 16) and args[4] is None, call
        if "view" in call:
            spec = args[5]._obj   # (byref's object: the spec the call built)
            assert isinstance(spec, _ViewSpec)
            got = (spec.planes_dev, spec.viewer_attrs_dev, spec.env_attrs_dev)
            assert t.address in got + (args[3],) and spec.dtype == (3 if arg == "codes" else 0) and spec.view_radius == 4, call
        else:
            assert t.address in (args[3], args[5], args[8], args[9]), (call, arg)
            assert args[6] == (3 if arg == "codes" else 0) and args[7] == int("per_agent" in call), (call, arg)


def test_element_type_comes_from_the_planes():
    env = _handle()
    mv = Duck((N, 4), I32)
    for dtype, code in (("torch.uint8", 0), ("torch.float16", 1), ("torch.float32", 2)):
        for per_agent in (False, True):
            planes = Duck((N, 4, 16, 11, 11) if per_agent else (N, 16, 11, 11), dtype)
            a, e = Duck((N, 4, 8), I32), Duck((N, 4), I32)
            env.step_device_range(16, 4, mv, planes=planes, per_agent=per_agent, agent_attrs=a, env_attrs=e)
            (entry, args), = env._lib.calls
            env._lib.calls.clear()
            assert entry == "pom_batch_step_device_range"
            assert args[1:] == (16, 4, mv.address, None, planes.address, code, int(per_agent), a.address, e.address)
    env.step_device_range(0, N, mv)   # no observation
    assert env._lib.calls.pop()[1][1:] == (0, N, mv.address, None, None, 0, 0, None, None)


def test_contradictions_and_ranges_outside_the_batch_are_refused():
    env = _handle()
    mv, codes, planes = Duck((N, 4), I32), Duck((N, 5, 11, 11), U8), Duck((N, 16, 11, 11), U8)
    attrs = Duck((N, 4, 8), I32)
    for kw in (dict(codes=codes, planes=planes), dict(codes=codes, per_agent=True), dict(agent_attrs=attrs), dict(per_agent=True),
               dict(env_attrs=Duck((N, 4), I32)), dict(planes=planes, viewer_attrs=Duck((N, 4, 12), I32)),
               dict(planes=Duck((N, 4, 16, 11, 11), U8), view_radius=4, agent_attrs=attrs), dict(view_radius=4),
               dict(planes=Duck((N, 4, 16, 11, 11), U8), view_radius=11)):
        with pytest.raises(ValueError):
            env.step_device_range(0, 16, mv, **kw)
    for first, count in ((-16, 16), (0, N + 1), (16, N), (N, 1), (0, -1)):
        with pytest.raises(ValueError, match="outside the batch"):
            env.step_device_range(first, count, mv)
    assert not env._lib.calls


def test_raw_addresses_pass_unchecked():
    """as in step_device: an integer is a device address the caller vouches for (planes then are uint8)"""
    env = _handle()
    env.step_device_range(0, 16, 0x1000, None, None, 0x2000, per_agent=True, agent_attrs=0x3000, env_attrs=0x4000)
    assert env._lib.calls.pop()[1][1:] == (0, 16, 0x1000, None, 0x2000, 0, 1, 0x3000, 0x4000)
    env.step_device_range(0, 16, 0x1000, 0x77, 0x2000)
    assert env._lib.calls.pop()[1][1:] == (0, 16, 0x1000, 0x77, 0x2000, 3, 0, None, None)


# ---- every other row of the table: torch and the library stood in for ---------------------------------------------------------------
def _all_rows(env):
    return range_rows(env, I32, U8, Duck) + other_rows(env, I8, I32, I64, U8, Duck)


def test_every_refused_row_of_the_table_reaches_no_library_function(monkeypatch):
    monkeypatch.setitem(sys.modules, "torch", W.standin_torch())
    env = _handle()
    rows = _all_rows(env)
    assert {r[0].split("(")[0] for r in rows} == {"step_device_range", "step_device", "step_device_many", "copy_envs", "observe", "forecast",
                                                   "move_safety", "rollout", "rollout_jobs", "expand", "move_table"}
    wrong, n = [], 0
    for call, arg, name, dtype, shape, free, fn in rows:
        for what, t in _bad(dtype, shape, free):
            n += 1
            try:
                fn(t)
                wrong.append(f"{call} {arg}, {what}: accepted")
            except ValueError as e:
                if name not in str(e):
                    wrong.append(f"{call} {arg}, {what}: the text does not name {name!r}: {e}")
            except Exception as e:  # noqa: BLE001 (every row is reported)
                wrong.append(f"{call} {arg}, {what}: {type(e).__name__} instead of ValueError: {e}")
            if env._lib.calls:
                wrong.append(f"{call} {arg}, {what}: reached {env._lib.calls[0][0]}")
                env._lib.calls.clear()
    assert n == sum(len(list(_bad(r[3], r[4], r[5]))) for r in rows) and n > 200
    assert not wrong, f"{len(wrong)} of {n} rows:\n" + "\n".join(wrong)


# where a right tensor's address must arrive: the entry point, and the argument's index or the spec's field
_ARRIVES = {
    ("step_device", "moves"): ("pom_batch_step_device", 1), ("step_device_many", "moves"): ("pom_batch_step_device_many", 1),
    ("copy_envs", "src"): ("pom_batch_copy_envs_device", 1), ("observe", "out"): ("pom_batch_observe", 1),
    ("forecast", "moves"): ("pom_batch_forecast", "moves_dev"), ("forecast", "out[flame_tick]"): ("pom_batch_forecast", "flame_tick_dev"),
    ("forecast", "out[agent_tick]"): ("pom_batch_forecast", "agent_tick_dev"), ("forecast", "out[ubflags]"): ("pom_batch_forecast", "ubflags_dev"),
    ("move_safety", "moves"): ("pom_batch_move_safety", "moves_dev"), ("move_safety", "out[death_tick]"): ("pom_batch_move_safety", "death_tick_dev"),
    ("move_safety", "out[escape_tick]"): ("pom_batch_move_safety", "escape_tick_dev"),
    ("rollout", "moves"): ("pom_batch_rollout", "moves_dev"), ("rollout", "out"): ("pom_batch_rollout", "result_dev"),
    ("rollout(simple=)", "moves"): ("pom_batch_rollout_policy", "moves_dev"),
    ("rollout_jobs", "src"): ("pom_batch_rollout_jobs", "src_dev"), ("rollout_jobs", "moves"): ("pom_batch_rollout_jobs", "moves_dev"),
    ("rollout_jobs", "out"): ("pom_batch_rollout_jobs", "result_dev"),
    ("expand", "src"): ("pom_batch_expand", "src_dev"), ("expand", "moves"): ("pom_batch_expand", "moves_dev"),
    ("expand", "out"): ("pom_batch_expand", "result_dev"), ("expand", "codes"): ("pom_batch_expand", "planes_dev"),
    ("expand", "planes"): ("pom_batch_expand", "planes_dev"), ("expand(per_agent)", "planes"): ("pom_batch_expand", "planes_dev"),
}


def test_every_right_tensor_of_the_other_calls_reaches_the_one_entry_point(monkeypatch):
    monkeypatch.setitem(sys.modules, "torch", W.standin_torch())
    env = _handle()
    rows = [r for r in other_rows(env, I8, I32, I64, U8, Duck) if r[0] != "move_table"]   # (its good path is real tensor arithmetic)
    assert {(r[0], r[1]) for r in rows} == set(_ARRIVES)
    for call, arg, name, dtype, shape, _, fn in rows:
        t = Duck(shape, dtype)
        fn(t)
        (entry, args), = env._lib.calls
        env._lib.calls.clear()
        want_entry, where = _ARRIVES[call, arg]
        assert entry == want_entry, (call, arg)
        if isinstance(where, int):
            assert args[where] == t.address and [a for a in args if a == t.address] == [t.address], (call, arg)
        else:
            spec = args[1]._obj   # (byref's object: the spec the call built)
            assert [f for f, *_ in spec._fields_ if getattr(spec, f) == t.address] == [where], (call, arg)
            assert spec.struct_size == C.sizeof(spec), (call, arg)
        if call.startswith("expand"):
            assert (spec.dtype, spec.per_agent) == (3 if arg == "codes" else 0, int("per_agent" in call)), (call, arg)


def test_expand_reads_the_element_type_by_name_and_refuses_addresses(monkeypatch):
    """as observe and step_device_range do: anything with a dtype that names uint8 / float16 / float32 serves as planes; a raw address
    does not, for codes or planes"""
    monkeypatch.setitem(sys.modules, "torch", W.standin_torch())
    env = _handle()
    src, mv = Duck((5,), I64), Duck((5, 4), I32)
    for dtype, code in (("uint8", 0), ("numpy.float16", 1), ("torch.float32", 2)):
        planes = Duck((N, 16, 11, 11), dtype)
        env.expand(src, mv, planes=planes, attrs=False)
        spec = env._lib.calls.pop()[1][1]._obj
        assert (spec.planes_dev, spec.dtype, spec.per_agent) == (planes.address, code, 0)
    for kw in (dict(planes=0x2000), dict(codes=0x2000), dict(planes=Duck((N, 16, 11, 11), "torch.int8"))):
        with pytest.raises(ValueError, match="codes|planes"):
            env.expand(src, mv, **kw)
    assert not env._lib.calls
