"""BatchEnvironment without a GPU, a library or torch: what stands in for each, and the fixed list of calls whose way into the library
is on record in tests/golden/wrapper_calls.json.

- `Duck`: what the wrapper looks at in a device tensor (data_ptr / shape / dtype / is_contiguous / device), with an address that must
  never be followed.  `Recorder`: the loaded library, every function of which exists, returns POM_OK and is written down.
- `standin_torch()`: a module to put into sys.modules as "torch": dtype names, `device`, and `empty` returning a Duck with `fill_`.
- `handle()`: a BatchEnvironment made with __new__ whose `_ordered` does nothing but say that it was entered.
- `play(module)`: plays the fixed list of calls (`_calls()`) on `module`'s BatchEnvironment and functions and returns, per call, what
  reached the library — the entry point, the scalar arguments, every spec as a dict of its fields — with addresses written by role: a caller's tensor by its argument
  name, a tensor the call allocated by where the call returns it (`ret[1]`, `ret['death_tick']`), a `fill_` as an event, a refusal as
  [class, the argument named].

Run as a script it plays the list on the batch.py of a scratch package and writes the record:
    python tests/wrapper_standin.py PACKAGE_DIR OUT.json     (PACKAGE_DIR: a directory holding batch.py, state.py and what they import)
The committed record was made this way from the parent commit's batch.py, not from the code under test."""
import contextlib
import ctypes as C
import importlib
import importlib.util
import json
import os
import sys
import types
from types import SimpleNamespace

import numpy as np

N, M = 20, 7   # envs (one whole tile of 16 and a short one); jobs of the list-driven calls
I8, I32, I64, U8, F16, F32 = ("torch." + d for d in ("int8", "int32", "int64", "uint8", "float16", "float32"))


class Duck:
    """what _device_tensor looks at, and an address that must never be followed"""
    _next = 0x7E0000000000

    def __init__(self, shape, dtype, contiguous=True, device="cuda", role=None, events=None):
        self.shape, self.dtype, self._contiguous = tuple(shape), dtype, contiguous
        self.device = SimpleNamespace(type=device, index=0 if device == "cuda" else None)
        Duck._next += 1 << 24
        self.address, self.role, self._events = Duck._next, role, events

    def is_contiguous(self):
        return self._contiguous

    def data_ptr(self):
        return self.address

    def fill_(self, value):
        if self._events is not None:
            self._events.append(("fill_", self, value))
        return self

    def to(self, device):   # (torch.from_numpy(a).to(dev) of expand()'s numpy arguments)
        return self


class Recorder:
    """stands in for the loaded library: every function exists, returns POM_OK and is written down"""

    def __init__(self, calls=None):
        self.calls = [] if calls is None else calls

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def standin_torch():
    """a module that serves as torch where torch only owns device memory; what its tensors are filled with goes to its `events`"""
    t = types.ModuleType("torch")
    t.events = []
    for d in ("int8", "int32", "int64", "uint8", "float16", "float32"):
        setattr(t, d, "torch." + d)
    t.device = lambda kind, index=None: SimpleNamespace(type=kind, index=index)
    t.empty = lambda shape, dtype=None, device=None: Duck(shape, dtype, events=t.events)
    t.from_numpy = lambda a: Duck(a.shape, "torch." + a.dtype.name, role=f"a copy of numpy {a.dtype.name}{list(a.shape)}", events=t.events)
    t.as_tensor = lambda raw, device=None: Duck(raw.__cuda_array_interface__["shape"], "torch.int32", events=t.events)   # (moves_tensor)
    return t


def handle(cls, lib=None, n=N, events=None):
    """a `cls` (BatchEnvironment) that was never created: no library handle (close() does nothing), `lib` in place of the library"""
    env = cls.__new__(cls)
    env._lib, env._h, env._views, env._tapes, env.n, env.device = Recorder() if lib is None else lib, C.c_void_p(), [], [], n, 0

    @contextlib.contextmanager
    def ordered(back=True, tensor=None):
        if events is not None:
            events.append(("_ordered", back, tensor))
        yield
    env._ordered = ordered
    return env


# ---- the fixed list of calls ----------------------------------------------------------------------------------------------------
# (id, callee, args, kwargs[, the argument a refusal must name]).  A T(...) is a caller's tensor, made anew for each call and known in
# the record by its name; callee "name": the handle's method, "live.name": the same on a handle that is not null, "module.name": the
# module's function or class.  safe_moves() and move_table() go on from their library call with real tensor arithmetic, which no stand-in
# does: safe_moves is covered by move_safety's rows and its own refusal, move_table by its refusals.
class T:
    def __init__(self, name, shape, dtype, **kw):
        self.name, self.shape, self.dtype, self.kw = name, shape, dtype, kw


def _obs_shape(layout, form):
    return (N,) + ((4,) if form != "plain" else ()) + ((5, 11, 11) if layout == "codes" else (16, 11, 11))


def _calls():
    mv = lambda: T("moves", (N, 4), I32)  # noqa: E731
    c = []
    # every call that takes no tensor: once with defaults, once with every optional argument set
    for name, variants in (
            ("generate", [((11,), {})]), ("episodes", [((), {}), ((4, 9), {})]), ("get_state", [((), {}), ((4, 9), {})]),
            ("snapshot", [((), {})]), ("step_random", [((5,), {}), ((5, 2, 7, 3), {})]),
            ("policy_simple", [((5,), {}), ((5, True), {})]), ("step_policy", [((), {})]), ("step_simple", [((5,), {}), ((5, 3), {})]),
            ("policy_memory", [((), {}), ((4, 9), {})]), ("set_tick", [((77,), {})]), ("status", [((), {}), ((4, 9), {})]),
            ("last_results", [((), {}), ((4, 9), {})]), ("get_terminal_state", [((), {}), ((4, 9), {})]), ("is_done", [((), {})]),
            ("is_draw", [((), {})]), ("get_winner", [((), {})]), ("chain_stats", [((), {})]), ("counters", [((), {})]),
            ("counters_into", [((0x5000,), {})]), ("reset_counters", [((), {})]), ("sync", [((), {})]), ("flush", [((), {})]),
            ("fork", [((), {})]), ("set_streams", [((2,), {})]), ("profile", [((True,), {})]), ("profile_read", [((), {})]),
            ("launch_shape", [((), {})]), ("issue_info", [((), {})]), ("device_view", [((), {})]), ("moves_tensor", [((), {})]),
            ("stream_handle", [((), {})]), ("close", [((), {})]), ("live.close", [((), {})]), ("live.stream_handle", [((), {})]),
            ("module.BatchEnvironment", [((N,), {}), ((N, 1, 0, 2, 800, 3000000000, 0x77, 32, 3, 1, True, 4000000001, 4), {})]),
            ("module.chain_litmus", [((4, 5, 2), {}), ((4, 5, 2, 1), {})])):
        c += [(f"{name} #{i}", name, a, k) for i, (a, k) in enumerate(variants)]
    c += [("make_game", "make_game", ("a state",), {}), ("make_game, first", "make_game", ("a state", 5), {}),
          ("step", "step", (np.zeros((N, 4), dtype=np.int64),), {}),
          ("step, wrong shape", "step", (np.zeros((N, 3), dtype=np.int32),), {}, "moves"),
          ("restore, mask", "restore", (np.arange(N) % 3 == 0,), {}), ("restore, indices", "restore", ([17, 3, 3, 9],), {}),
          ("restore, nobody", "restore", ([],), {}), ("restore, outside", "restore", ([N],), {}, "indices"),
          ("restore, short mask", "restore", (np.zeros(N - 1, dtype=bool),), {}, "mask"),
          ("copy_envs, numpy", "copy_envs", (np.array([3, -1, 5]),), {}),
          ("copy_envs, numpy, everything set", "copy_envs", (np.array([3, -1, 5]), 2), dict(from_snapshot=True, set_snapshot=True, count=3)),
          ("copy_envs, numpy, count differs", "copy_envs", (np.array([3, -1, 5]),), dict(count=4), "count"),
          ("copy_envs, floats", "copy_envs", (np.zeros(3),), {}, "src"),
          ("copy_envs, tensor", "copy_envs", (T("src", (M,), I64), 4), dict(set_snapshot=True)),
          ("copy_envs, tensor, count", "copy_envs", (T("src", (M,), I64),), dict(count=M, from_snapshot=True)),
          ("copy_envs, tensor, count differs", "copy_envs", (T("src", (M,), I64),), dict(count=M + 1), "src"),
          ("copy_envs, address", "copy_envs", (0x6000, 2), dict(count=5)),
          ("copy_envs, address without count", "copy_envs", (0x6000,), {}, "count"),
          ("step_device", "step_device", (mv(),), {}), ("step_device, address", "step_device", (0x1000,), {}),
          ("step_device, int64", "step_device", (T("moves", (N, 4), I64),), {}, "moves"),
          ("step_device_many", "step_device_many", (T("moves", (3, N, 4), I32),), {}),
          ("step_device_many, ticks", "step_device_many", (T("moves", (3, N, 4), I32), 3), {}),
          ("step_device_many, ticks differ", "step_device_many", (T("moves", (3, N, 4), I32), 4), {}, "moves"),
          ("step_device_many, address", "step_device_many", (0x1000, 6), {}),
          ("step_device_many, address without ticks", "step_device_many", (0x1000,), {}, "ticks"),
          ("module.bench_policy", "module.bench_policy", (None, mv(), 0, 16, 5), {}),
          ("module.bench_policy, everything set", "module.bench_policy", (T("codes", (N, 5, 11, 11), U8), mv(), 16, 4, -1, 0x77), {}),
          ("module.step_one", "module.step_one", ("a state", [1, 2, 3, 4]), {}),
          ("module.env_step_one", "module.env_step_one", ("a state", [1, 2, 3, 4]), {}),
          ("module.env_step_one, max_steps", "module.env_step_one", ("a state", [1, 2, 3, 4], 800), {})]

    # the observation: every legal combination of {uint8, float16, float32, codes} x {plain, per_agent, view_radius} x attrs on / off
    for layout, dtype in (("uint8", U8), ("float16", F16), ("float32", F32), ("codes", U8)):
        for form in ("plain", "per_agent", "view"):
            legal = not (layout == "codes" and form == "per_agent")
            shape, what = _obs_shape(layout, form), f"{layout}, {form}"
            form_kw = {"plain": {}, "per_agent": dict(per_agent=True), "view": dict(view_radius=4)}[form]
            obs = lambda: {"codes" if layout == "codes" else "planes": T("codes" if layout == "codes" else "planes", shape, dtype)}  # noqa: E731
            for attrs in (True, False):
                tail = (what + ("" if attrs else ", no attrs"),) if legal else (what, "per-agent")
                if not legal and not attrs:
                    continue
                c.append(("observe: " + tail[0], "observe", (), dict(dtype=layout, attrs=attrs, **form_kw), *tail[1:]))
                c.append(("observe(out=): " + tail[0], "observe", (), dict(dtype=layout, attrs=attrs, out=T("out", shape, dtype), **form_kw), *tail[1:]))
                c.append(("step_device_observe: " + tail[0], "step_device_observe", (mv(),), dict(dtype=layout, attrs=attrs, **form_kw), *tail[1:]))
                a_name, width = ("viewer_attrs", 12) if form == "view" else ("agent_attrs", 8)
                given = {a_name: T(a_name, (N, 4, width), I32), "env_attrs": T("env_attrs", (N, 4), I32)} if attrs else {}
                c.append(("step_device_range: " + tail[0], "step_device_range", (0, 16, mv()), {**obs(), **form_kw, **given}, *tail[1:]))
                if layout in ("uint8", "codes"):   # a raw address has no element type: planes then are uint8
                    raw = {k: 0x2000 + 0x1000 * i for i, k in enumerate({**obs(), **given})}
                    c.append(("step_device_range, addresses: " + tail[0], "step_device_range", (16, 4, 0x1000, 0x77), {**raw, **form_kw}, *tail[1:]))
                if form != "view":
                    c.append(("expand: " + tail[0], "expand", (T("src", (M,), I64), T("moves", (M, 4), I32), 3),
                              dict(attrs=attrs, **obs(), **({} if form == "plain" else form_kw)), *tail[1:]))
    planes, views = lambda: T("planes", (N, 16, 11, 11), U8), lambda: T("planes", (N, 4, 16, 11, 11), U8)  # noqa: E731
    codes = lambda: T("codes", (N, 5, 11, 11), U8)  # noqa: E731
    c += [("step_device_range", "step_device_range", (0, N, mv()), {}),
          ("step_device_range, a torch stream", "step_device_range", (0, 16, mv(), SimpleNamespace(cuda_stream=0x77)), {}),
          ("step_device_observe, out and everything set", "step_device_observe", (mv(), True, "float16", False, T("out", (N, 4, 16, 11, 11), F16), 0), {})]
    # every contradiction the docstrings name
    for what, kw, arg in (("codes and planes", dict(codes=codes(), planes=planes()), "codes"),
                          ("codes, per_agent", dict(codes=codes(), per_agent=True), "per-agent"),
                          ("view_radius, per_agent=False", dict(planes=views(), view_radius=4, per_agent=False), "per_agent"),
                          ("view_radius 11", dict(planes=views(), view_radius=11), "view_radius"),
                          ("view_radius -1", dict(planes=views(), view_radius=-1), "view_radius"),
                          ("viewer_attrs without view_radius", dict(planes=planes(), viewer_attrs=T("viewer_attrs", (N, 4, 12), I32)), "viewer_attrs"),
                          ("agent_attrs with view_radius", dict(planes=views(), view_radius=4, agent_attrs=T("agent_attrs", (N, 4, 8), I32)), "agent_attrs"),
                          ("agent_attrs alone", dict(agent_attrs=T("agent_attrs", (N, 4, 8), I32)), "agent_attrs"),
                          ("env_attrs alone", dict(env_attrs=T("env_attrs", (N, 4), I32)), "env_attrs"),
                          ("per_agent alone", dict(per_agent=True), "per_agent"), ("view_radius alone", dict(view_radius=4), "view_radius"),
                          ("planes of int32", dict(planes=T("planes", (N, 16, 11, 11), I32)), "planes"),
                          ("planes of the range's size", dict(planes=T("planes", (16, 16, 11, 11), U8)), "planes")):
        c.append(("step_device_range refuses: " + what, "step_device_range", (0, 16, mv()), kw, arg))
    for first, count in ((-16, 16), (0, N + 1), (16, N), (N, 1), (0, -1)):
        c.append((f"step_device_range refuses: [{first}, {first + count})", "step_device_range", (first, count, mv()), {}, "outside the batch"))
    for what, kw, arg in (("per_agent=False with view_radius", dict(per_agent=False, view_radius=4), "per_agent"),
                          ("dtype int32", dict(dtype="int32"), "dtype"), ("view_radius 11", dict(view_radius=11), "view_radius"),
                          ("out of another shape", dict(out=T("out", (N, 4, 16, 11, 11), U8)), "out"),
                          ("out of another type", dict(dtype="float16", out=T("out", (N, 16, 11, 11), F32)), "out")):
        c.append(("observe refuses: " + what, "observe", (), kw, arg))
    c.append(("step_device_observe refuses: moves", "step_device_observe", (T("moves", (N, 3), I32),), {}, "moves"))
    job = lambda: (T("src", (M,), I64), T("moves", (M, 4), I32))  # noqa: E731
    for what, a, kw, arg in (("codes and planes", job(), dict(codes=codes(), planes=planes()), "codes"),
                             ("codes, per_agent", job(), dict(codes=codes(), per_agent=True), "per-agent"),
                             ("planes of int32", job(), dict(planes=T("planes", (N, 16, 11, 11), I32)), "planes"),
                             ("planes as an address", job(), dict(planes=0x2000), "planes"),
                             ("codes as an address", job(), dict(codes=0x2000), "codes"),
                             ("a range outside the batch", job() + (N - M + 1,), {}, "outside the batch"),
                             ("first < 0", job() + (-1,), {}, "outside the batch"),
                             ("numpy floats", (np.zeros(M), np.zeros((M, 4), dtype=np.int32)), {}, "src"),
                             ("moves of another length", (T("src", (M,), I64), T("moves", (M + 1, 4), I32)), {}, "moves")):
        c.append(("expand refuses: " + what, "expand", a, kw, arg))
    c += [("expand", "expand", job(), {}), ("expand, out", "expand", job() + (N - M,), dict(out=T("out", (M,), I32))),
          ("expand, numpy", "expand", (np.arange(M), np.zeros((M, 4), dtype=np.int16)), {}),
          ("expand, no jobs", "expand", (T("src", (0,), I64), T("moves", (0, 4), I32)), dict(planes=planes())),
          ("expand, per_agent without an observation", "expand", job(), dict(per_agent=True))]

    # the look-ahead calls
    out3 = lambda: {"flame_tick": T("out['flame_tick']", (N, 11, 11), U8), "agent_tick": T("out['agent_tick']", (N, 4), I32),  # noqa: E731
                    "ubflags": T("out['ubflags']", (N,), I32)}
    c += [("forecast", "forecast", (4,), {}), ("forecast, everything set", "forecast", (32, mv(), out3(), True, True), {}),
          ("forecast, flames only", "forecast", (1,), dict(agent_ticks=False)),
          ("forecast, part of out", "forecast", (4,), dict(out={"agent_tick": T("out['agent_tick']", (N, 4), I32)}, ubflags=True)),
          ("forecast refuses: horizon 0", "forecast", (0,), {}, "horizon"), ("forecast refuses: horizon 33", "forecast", (33,), {}, "horizon"),
          ("forecast refuses: moves", "forecast", (4, T("moves", (N, 4), I64)), {}, "moves"),
          ("forecast refuses: moves as an address", "forecast", (4, 0x1000), {}, "moves"),
          ("forecast refuses: out", "forecast", (4,), dict(out={"flame_tick": T("out['flame_tick']", (N, 11, 11), I32)}), "flame_tick")]
    out2 = lambda: {"death_tick": T("out['death_tick']", (N, 4, 6), I8), "escape_tick": T("out['escape_tick']", (N, 4, 6), I8)}  # noqa: E731
    c += [("move_safety", "move_safety", (4,), {}), ("move_safety, everything set", "move_safety", (32, [1, 3], mv(), out2(), True, True), {}),
          ("move_safety, some agents, new tensors", "move_safety", (4, 0b0101), {}),
          ("move_safety, some agents, one of out", "move_safety", (4, [2]), dict(out={"escape_tick": T("out['escape_tick']", (N, 4, 6), I8)})),
          ("move_safety, death only", "move_safety", (4,), dict(escape=False)), ("move_safety, escape only", "move_safety", (4,), dict(death=False)),
          ("move_safety refuses: horizon", "move_safety", (33,), {}, "horizon"), ("move_safety refuses: nobody", "move_safety", (4, []), {}, "agents"),
          ("move_safety refuses: agent 4", "move_safety", (4, [4]), {}, "agents"), ("move_safety refuses: mask 16", "move_safety", (4, 16), {}, "agents"),
          ("move_safety refuses: nothing to compute", "move_safety", (4,), dict(death=False, escape=False), "escape"),
          ("move_safety refuses: moves", "move_safety", (4, None, T("moves", (N, 5), I32)), {}, "moves"),
          ("move_safety refuses: out", "move_safety", (4,), dict(out={"death_tick": T("out['death_tick']", (N, 4, 6), I32)}), "death_tick"),
          ("safe_moves refuses: horizon", "safe_moves", (0,), {}, "horizon")]
    c += [("rollout", "rollout", (4, 2, 1), {}), ("rollout, moves", "rollout", (4, 2, -1, 2, mv()), {}),
          ("rollout, everything set", "rollout", (1024, 256, 1 << 70, 0, mv(), T("out", (256, N), I32)), dict(simple=[0, 2], first=0b1000, fresh_agents=True)),
          ("rollout, simple", "rollout", (4, 2, 1), dict(simple=3)), ("rollout, fresh agents", "rollout", (4, 2, 1), dict(fresh_agents=True)),
          ("rollout, first without agents", "rollout", (4, 2, 1), dict(first=[])), ("rollout, moves and simple", "rollout", (4, 2, 1, 1, mv()), dict(simple=[1])),
          ("rollout refuses: horizon", "rollout", (1025, 2, 1), {}, "horizon"), ("rollout refuses: samples", "rollout", (4, 257, 1), {}, "samples"),
          ("rollout refuses: dist", "rollout", (4, 2, 1, 3), {}, "dist"), ("rollout refuses: first without moves", "rollout", (4, 2, 1), dict(first=[1]), "first"),
          ("rollout refuses: simple", "rollout", (4, 2, 1), dict(simple=[4]), "simple"), ("rollout refuses: moves", "rollout", (4, 2, 1, 1, T("moves", (N,), I32)), {}, "moves"),
          ("rollout refuses: out", "rollout", (4, 2, 1), dict(out=T("out", (3, N), I32)), "out"),
          ("rollout_jobs", "rollout_jobs", (T("src", (M,), I64), 4, 2, 1), {}),
          ("rollout_jobs, everything set", "rollout_jobs", (T("src", (M,), I64), 1024, 256, -1, 2, T("moves", (M, 4), I32), T("out", (256, M), I32)),
           dict(simple=0b0110, first=[0], fresh_agents=True)),
          ("rollout_jobs, moves", "rollout_jobs", (T("src", (M,), I64), 4, 2, 1), dict(moves=T("moves", (M, 4), I32))),
          ("rollout_jobs, no jobs", "rollout_jobs", (T("src", (0,), I64), 4, 2, 1), dict(moves=T("moves", (0, 4), I32))),
          ("rollout_jobs refuses: src", "rollout_jobs", (T("src", (M, 1), I64), 4, 2, 1), {}, "src"),
          ("rollout_jobs refuses: moves", "rollout_jobs", (T("src", (M,), I64), 4, 2, 1), dict(moves=T("moves", (N, 4), I32)), "moves"),
          ("rollout_jobs refuses: out", "rollout_jobs", (T("src", (M,), I64), 4, 2, 1), dict(out=T("out", (2, N), I32)), "out"),
          ("rollout_jobs refuses: first without moves", "rollout_jobs", (T("src", (M,), I64), 4, 2, 1), dict(first=1), "first"),
          ("move_table refuses: agent", "move_table", (4, 4, 2, 1), {}, "agent"),
          ("move_table refuses: others", "move_table", (0, 4, 2, 1), dict(others=T("others", (N, 3), I32)), "others")]
    ids = [x[0] for x in c]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return c


# ---- playing them ---------------------------------------------------------------------------------------------------------------
def _roles(ret, path, into):
    """the tensors in what a call returned, by where it returns them"""
    if isinstance(ret, Duck):
        into.setdefault(ret.address, ret.role or path)
    elif isinstance(ret, (tuple, list)):
        for i, r in enumerate(ret):
            _roles(r, f"{path}[{i}]", into)
    elif isinstance(ret, dict):
        for k, r in ret.items():
            _roles(r, f"{path}[{k!r}]", into)


def _plain(v, roles):
    """a value that reached the library, or one that a call returned, as JSON with addresses written by role"""
    if isinstance(v, Duck):
        return {"tensor": roles.get(v.address, "?"), "shape": list(v.shape), "dtype": v.dtype}
    if isinstance(v, (bool, type(None), str, float)):
        return v
    if isinstance(v, (int, np.integer)):
        v = int(v)
        return roles.get(v, "a host buffer" if v >= 1 << 32 else v)   # (the addresses the list passes raw are small)
    if isinstance(v, np.ndarray):
        return {"numpy": v.dtype.name if v.dtype.names is None else "STATE", "shape": list(v.shape)}
    if isinstance(v, C.c_void_p):
        return "the handle"
    if isinstance(v, C.Structure):
        return {type(v).__name__: {f: _plain(getattr(v, f), roles) for f, *_ in v._fields_}}
    if isinstance(v, C.Array):
        return [_plain(x, roles) for x in v]
    if hasattr(v, "_obj"):   # byref
        return _plain(v._obj, roles) if isinstance(v._obj, C.Structure) else "&" + type(v._obj).__name__
    if isinstance(v, (tuple, list)):
        return [_plain(x, roles) for x in v]
    if isinstance(v, dict):
        return {k: _plain(x, roles) for k, x in v.items()}
    return type(v).__name__


def play(module, only=None):
    """the fixed list of calls played on `module` (a batch.py), "torch" in sys.modules being standin_torch's: {id: the record of the call}"""
    from_state = importlib.import_module(module.__name__.rsplit(".", 1)[0] + ".state")
    record = {}
    for cid, callee, args, kwargs, *named in _calls():
        if only is not None and cid not in only:
            continue
        events, roles = [], {}
        sys.modules["torch"].events = events

        def real(a):
            if isinstance(a, T):
                d = Duck(a.shape, a.dtype, role=a.name, events=events, **a.kw)
                roles[d.address] = a.name
                return d
            if isinstance(a, dict):
                return {k: real(x) for k, x in a.items()}
            return from_state.new_states(1) if isinstance(a, str) and a == "a state" else a
        lib = Recorder(events)
        env = handle(module.BatchEnvironment, lib, events=events)
        if callee.startswith("live."):
            env._h, callee = C.c_void_p(0x4000), callee[5:]
        saved, module.load_library = module.load_library, lambda: lib
        try:
            fn = getattr(module, callee[7:]) if callee.startswith("module.") else getattr(env, callee)
            try:
                ret = fn(*[real(a) for a in args], **{k: real(v) for k, v in kwargs.items()})
            except (ValueError, AssertionError) as e:
                reached = [ev[0] for ev in events if ev[0] not in ("fill_", "_ordered")]
                record[cid] = {"refused": [type(e).__name__, named[0] if named and named[0] in str(e) else str(e)], "reached": reached}
                continue
        finally:
            module.load_library = saved
        if isinstance(ret, module.BatchEnvironment):   # the constructor's: what it made of its arguments
            env, ret = ret, {"n": ret.n, "device": ret.device}
        _roles(ret, "ret", roles)
        out = []
        for name, *rest in events:
            if name == "fill_":
                out.append(["fill_", _plain(rest[0], roles)["tensor"], rest[1]])
            elif name == "_ordered":
                out.append(["_ordered", {"back": rest[0], "tensor": _plain(rest[1], roles)}])
            else:
                out.append([name, _plain(rest[0], roles)])
        record[cid] = {"events": out, "returns": _plain(ret, roles), "tapes": len(env._tapes), "views": len(env._views), "handle": bool(env._h)}
    return record


def load_scratch_package(directory, name="pom_scratch_parent"):
    """the package in `directory` (its batch.py, state.py, ...) imported under `name`; returns its batch module"""
    spec = importlib.util.spec_from_file_location(name, os.path.join(directory, "__init__.py"), submodule_search_locations=[directory])
    pkg = importlib.util.module_from_spec(spec)
    sys.modules[name] = pkg
    spec.loader.exec_module(pkg)
    return importlib.import_module(name + ".batch")


if __name__ == "__main__":
    directory, out_path = sys.argv[1:3]
    os.environ["POM_NO_TORCH"] = "1"
    sys.modules["torch"] = standin_torch()
    rec = play(load_scratch_package(os.path.abspath(directory)))
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(rec)} calls, {sum('refused' in r for r in rec.values())} of them refusals -> {out_path}")
