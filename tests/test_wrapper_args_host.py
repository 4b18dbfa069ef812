"""BatchEnvironment.step_device_range's argument checks without a GPU: the rows of tests/test_wrapper_args.py for that call, driven
against a BatchEnvironment made with __new__ whose library is a recording stand-in, with duck tensors (data_ptr / shape / dtype /
is_contiguous / device) in place of device tensors.  A refused row raises a ValueError that names the argument and reaches NO library
function — on a real handle it would have launched a kernel on a bad address —; a right tensor reaches exactly the one entry point,
with the addresses, the element type's code and per_agent it should.  The call makes no runtime call, so nothing here needs torch."""
import ctypes as C
from types import SimpleNamespace

import pytest

from pomcpp_amd.batch import BatchEnvironment, _ViewSpec
from tests.test_wrapper_args import N, range_rows

I32, U8 = "torch.int32", "torch.uint8"


class Duck:
    """what _device_tensor looks at, and an address that must never be followed"""
    _next = 0x7E0000000000

    def __init__(self, shape, dtype, contiguous=True, device="cuda"):
        self.shape, self.dtype, self._contiguous = tuple(shape), dtype, contiguous
        self.device = SimpleNamespace(type=device, index=0 if device == "cuda" else None)
        Duck._next += 1 << 24
        self.address = Duck._next

    def is_contiguous(self):
        return self._contiguous

    def data_ptr(self):
        return self.address


class Recorder:
    """stands in for the loaded library: every function exists, returns POM_OK and is written down"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def _handle():
    env = BatchEnvironment.__new__(BatchEnvironment)
    env._lib, env._h, env._views, env._tapes, env.n, env.device = Recorder(), C.c_void_p(), [], [], N, 0   # (a null handle: close() does nothing)
    return env


def _bad(dtype, shape):
    """tests/test_wrapper_args._bad as ducks: (what is wrong, tensor)"""
    yield "dtype", Duck(shape, "torch.int64" if dtype == I32 else I32)
    yield "dtype, float for bytes", Duck(shape, "torch.float64")
    yield "shape, one dimension more", Duck(shape + (2,), dtype)
    yield "shape, last dimension", Duck(shape[:-1] + (shape[-1] + 1,), dtype)
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
