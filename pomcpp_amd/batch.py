"""`BatchEnvironment` over the ctypes binding of libpom_batch.so (pomcpp_amd/_abi.py mirrors include/pom_batch.h).

`BatchEnvironment` mirrors `bboard::Environment` (/root/reference/include/bboard.hpp:541-644,
src/bboard/environment.cpp:48-213) for n concurrent games on one MI355X:

    reference (one game)                 here (n games)
    env.MakeGame(agents)                 env.make_game(states)            # states: STATE_DTYPE[n]
    env.Step()  -> act x4, bboard::Step  env.step(moves)                  # moves: int32[n,4], dead agents included
    env.IsDone() / IsDraw() / GetWinner  env.is_done() / is_draw() / get_winner()   # arrays of n
    env.GetState()                       env.get_state(first, count)      # STATE_DTYPE[count]

The library is the only stepper.  If it is missing or no HIP device is present, loading or
creating a batch raises — nothing falls back to the CPU.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import sys
import weakref
from typing import Optional

import numpy as np

from ._abi import (  # noqa: F401 (the binding's names are this module's too: callers import them from here)
    MODE_RAW, MODE_ENV, RESET_OFF, RESET_AT_START, RESET_AT_END, DIST_HARMLESS, DIST_RANDOM, DIST_STRESS,
    CNT_STEPS, CNT_EPISODES, CNT_RESETS, CNT_UB_TICKS, ISSUE_AUTO, ISSUE_DIRECT, ISSUE_THREADS, ISSUE_GRAPH, ISSUE_CHAIN,
    COPY_FROM_SNAPSHOT, COPY_SET_SNAPSHOT, UB_LOST_AGENT, UB_NULL_BOMB, UB_QUEUE_OVERFLOW, UB_REVERT_LOOP, UB_BAD_INDEX,
    UB_FLAME_QUEUE_RANGE, ROLLOUT_FRESH_AGENTS, RO_NONE, RO_ALIVE, RO_DONE, RO_DRAW, RO_TIMEOUT, RO_UB, RO_WINNER_SHIFT,
    RO_WINNER_MASK, RO_LENGTH_SHIFT, REACH_MAX_DIST, MEMORY_PLANES, MEMORY_AGE_NEVER, MEMORY_AGE_MAX, PomError, _Options, _ViewSpec, _ForecastSpec,
    _MoveSafetySpec, _ReachSpec, _MemorySpec, _ImagineSpec, _RolloutSpec, IMAGINE_SAMPLE, IMAGINE_PASSAGE, IMAGINE_BUILT, IMAGINE_DROPPED_BOMBS,
    IMAGINE_DROPPED_FLAMES, IMAGINE_NO_ROOM, IMAGINE_UNKNOWN_SHIFT, IMAGINE_DRAWN_SHIFT, _BoardLayout, _DealSpec, DEAL_START, DEAL_NEXT, DEAL_ALL,
    DEAL_MASK, DEAL_RESTARTED, DEAL_DONE, LAYOUT_NO_LANES, DEAL_DEALT, DEAL_FALLBACK, DEAL_ATTEMPTS_SHIFT, DEAL_BAD_SHIFT,
    _RolloutPolicySpec, _RolloutJobsSpec, _ExpandSpec, _MixedStepSpec, _StepEventsSpec, _CompactViewSpec, VIEW_CENTRED, EV_MOVE, EV_PLAYED, EV_ALIVE, EV_DIED, EV_MOVED, EV_LAID,
    EV_GAIN_BOMB, EV_GAIN_RANGE, EV_GAIN_KICK, EV_RESTARTED, EV_EXPLODED_SHIFT, EV_EXPLODED, EV_END, EV_WON, EV_DRAW, EV_TIMEOUT, EV_UB, _ptr, _spec, _view_spec, _forecast_spec, library_path, load_library, _check)
from .state import STATE_DTYPE


def _bounded(v, name: str, lo: int, hi: int) -> int:
    """`v` as an int of lo..hi"""
    if not lo <= int(v) <= hi:
        raise ValueError(f"{name} must be {lo}..{hi}")
    return int(v)


def _lookahead(horizon) -> int:
    """the horizon of forecast() and move_safety(), which play every tick of it on a scratch copy"""
    return _bounded(horizon, "horizon", 1, 32)


def _u64(seed) -> int:
    """a seed as the uint64 a spec carries"""
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def _job_ptrs(m: int, *tensors):
    """the addresses of a job list's arrays; no jobs: NULL pointers (an empty tensor has no address worth passing)"""
    return tuple(_ptr(t) if m else None for t in tensors)


def _dtype_name(dtype) -> str:
    """an element type by name: "uint8" for torch.uint8 as for the string"""
    return str(dtype).rsplit(".", 1)[-1]


_PLANE_CODES = {"uint8": 0, "float16": 1, "float32": 2}  # POM_OBS_U8 / F16 / F32; 3 = POM_OBS_CODES


def _agent_mask(v, name: str) -> int:
    """a mask int 0..15, or an iterable of agent ids 0..3"""
    if isinstance(v, (int, np.integer)) and not isinstance(v, bool):
        m = int(v)
        if not 0 <= m <= 15:
            raise ValueError(f"{name} must be a mask 0..15 or an iterable of agent ids 0..3")
        return m
    try:
        ids = [int(a) for a in v]
    except TypeError:
        raise ValueError(f"{name} must be a mask 0..15 or an iterable of agent ids 0..3") from None
    if any(not 0 <= a <= 3 for a in ids):
        raise ValueError(f"{name} must be a mask 0..15 or an iterable of agent ids 0..3")
    return sum(1 << a for a in set(ids))


def _compact_views(viewers, centred):
    """observe()'s, step_mixed()'s and step_events()'s `viewers` / `centred`: None for the four-view form (neither given), else the
    PomCompactViewSpec's (viewer_mask, flags) — `viewers` a mask int or an iterable of agent ids as `agents=` is elsewhere, not empty;
    None with `centred`: all four"""
    if viewers is None and not centred:
        return None
    mask = 15 if viewers is None else _agent_mask(viewers, "viewers")
    if mask == 0:
        raise ValueError("viewers names no agent: a compact view has at least one viewer")
    return mask, VIEW_CENTRED if centred else 0


def _rollout_args(horizon, samples, dist, moves, simple, first, fresh_agents, policy: bool = True):
    """rollout()'s and rollout_jobs()'s arguments checked: (horizon, samples, dist, simple_mask, first_mask, flags); without `policy`
    (pom_batch_rollout's playouts) the masks are 0"""
    horizon, samples = _bounded(horizon, "horizon", 1, 1024), _bounded(samples, "samples", 1, 256)
    if dist not in (DIST_HARMLESS, DIST_RANDOM, DIST_STRESS):
        raise ValueError("dist must be DIST_HARMLESS, DIST_RANDOM or DIST_STRESS")
    simple_mask = first_mask = 0
    if policy:
        simple_mask = 0 if simple is None else _agent_mask(simple, "simple")
        first_mask = (0 if moves is None else 0xF) if first is None else _agent_mask(first, "first")
        if first_mask and moves is None:
            raise ValueError("first names agents but moves is None")
    return horizon, samples, int(dist), simple_mask, first_mask, ROLLOUT_FRESH_AGENTS if fresh_agents else 0


def decode_rollout(result) -> dict:
    """The fields of rollout()'s result words (torch tensor or numpy array of any shape [...], int32 or uint32): `alive` bool
    [..., 4], `done`, `draw`, `timeout`, `ub` bool [...], `winner` (-1: nobody) and `length` (ticks played) int32 [...]; the same kind of
    array as the input, on its device.  Reductions are the caller's: decode_rollout(r)["alive"].float().mean(0) is the survival rate."""
    w = result
    if isinstance(w, np.ndarray):
        w = w.astype(np.int64) & 0xFFFFFFFF
        bits, i32 = w[..., None] >> np.arange(4) & 1, lambda a: a.astype(np.int32)  # noqa: E731
    else:
        import torch
        w = w.to(torch.int64) & 0xFFFFFFFF
        bits, i32 = w[..., None] >> torch.arange(4, device=w.device) & 1, lambda a: a.to(torch.int32)  # noqa: E731
    return {"alive": bits != 0, "done": (w & RO_DONE) != 0, "draw": (w & RO_DRAW) != 0, "timeout": (w & RO_TIMEOUT) != 0,
            "ub": (w & RO_UB) != 0, "winner": i32(((w & RO_WINNER_MASK) >> RO_WINNER_SHIFT) - 1), "length": i32(w >> RO_LENGTH_SHIFT)}


def decode_step_events(word) -> dict:
    """The fields of step_events()'s event words (torch tensor or numpy array of any shape [...], int32 or uint32; PomStepEventsSpec in
    include/pom_batch.h states the rule): `move` and `exploded` (own bombs that went off) int32 [...]; `played`, `alive`, `died`, `moved`,
    `laid`, `gain_bomb`, `gain_range`, `gain_kick`, `restarted`, `end`, `won`, `draw`, `timeout`, `ub` bool [...]; the same kind of array
    as the input, on its device.  The outcome words are rollout()'s: decode_rollout()."""
    w = word
    if isinstance(w, np.ndarray):
        w, i32 = w.astype(np.int64) & 0xFFFFFFFF, lambda a: a.astype(np.int32)  # noqa: E731
    else:
        import torch
        w, i32 = w.to(torch.int64) & 0xFFFFFFFF, lambda a: a.to(torch.int32)  # noqa: E731
    out = {"move": i32(w & EV_MOVE), "exploded": i32((w & EV_EXPLODED) >> EV_EXPLODED_SHIFT)}
    for name, bit in (("played", EV_PLAYED), ("alive", EV_ALIVE), ("died", EV_DIED), ("moved", EV_MOVED), ("laid", EV_LAID),
                      ("gain_bomb", EV_GAIN_BOMB), ("gain_range", EV_GAIN_RANGE), ("gain_kick", EV_GAIN_KICK), ("restarted", EV_RESTARTED),
                      ("end", EV_END), ("won", EV_WON), ("draw", EV_DRAW), ("timeout", EV_TIMEOUT), ("ub", EV_UB)):
        out[name] = (w & bit) != 0
    return out


def decode_imagine(word) -> dict:
    """The fields of imagine()'s result words (torch tensor or numpy array of any shape [...], int32 or uint32): `built`,
    `dropped_bombs`, `dropped_flames`, `no_room` bool [...], `unknown` (the never-seen cells of the view) int32 [...], `drawn` bool
    [..., 4] (agent a was placed by a draw); the same kind of array as the input, on its device.  A word of 0 is "no job"."""
    w = word
    if isinstance(w, np.ndarray):
        w = w.astype(np.int64) & 0xFFFFFFFF
        bits, i32 = (w >> IMAGINE_DRAWN_SHIFT)[..., None] >> np.arange(4) & 1, lambda a: a.astype(np.int32)  # noqa: E731
    else:
        import torch
        w = w.to(torch.int64) & 0xFFFFFFFF
        bits, i32 = (w >> IMAGINE_DRAWN_SHIFT)[..., None] >> torch.arange(4, device=w.device) & 1, lambda a: a.to(torch.int32)  # noqa: E731
    return {"built": (w & IMAGINE_BUILT) != 0, "dropped_bombs": (w & IMAGINE_DROPPED_BOMBS) != 0, "dropped_flames": (w & IMAGINE_DROPPED_FLAMES) != 0,
            "no_room": (w & IMAGINE_NO_ROOM) != 0, "unknown": i32((w >> IMAGINE_UNKNOWN_SHIFT) & 0xFF), "drawn": bits != 0}


def decode_deal(word) -> dict:
    """The fields of deal()'s result words (torch tensor or numpy array of any shape [...], int32 or uint32): `dealt`, `fallback` bool
    [...] (all 16 attempts were rejected: the board is the last one), `attempts` (used, 1..16) and `bad` (passages walled off from
    agent 0's cell) int32 [...]; the same kind of array as the input, on its device.  A word of 0: the env was not dealt."""
    w = word
    if isinstance(w, np.ndarray):
        w, i32 = w.astype(np.int64) & 0xFFFFFFFF, lambda a: a.astype(np.int32)  # noqa: E731
    else:
        import torch
        w, i32 = w.to(torch.int64) & 0xFFFFFFFF, lambda a: a.to(torch.int32)  # noqa: E731
    dealt = (w & DEAL_DEALT) != 0
    return {"dealt": dealt, "fallback": (w & DEAL_FALLBACK) != 0, "attempts": i32(((w >> DEAL_ATTEMPTS_SHIFT) & 0xFF) + dealt),
            "bad": i32((w >> DEAL_BAD_SHIFT) & 0xFF)}


class BoardLayout:
    """The counts of a dealt start board (PomBoardLayout, include/pom_batch.h): `num_rigid` rigid walls and `num_wood` woods (both even;
    the woods include the 12 of the lanes between neighbouring agents unless `no_lanes`), `num_items` woods that hide a power-up,
    `max_inaccessible` passages that may be walled off from agent 0's cell before an attempt is rejected.  The default is Pommerman's
    standard board: 36, 36, 20, 4.  A layout the library would refuse raises ValueError here."""
    __slots__ = ("num_rigid", "num_wood", "num_items", "max_inaccessible", "flags")

    def __init__(self, num_rigid: int = 36, num_wood: int = 36, num_items: int = 20, max_inaccessible: int = 4, no_lanes: bool = False):
        self.num_rigid, self.num_wood, self.num_items = int(num_rigid), int(num_wood), int(num_items)
        self.max_inaccessible, self.flags = int(max_inaccessible), LAYOUT_NO_LANES if no_lanes else 0
        lanes = 0 if no_lanes else 12
        for name in ("num_rigid", "num_wood"):
            if getattr(self, name) < 0 or getattr(self, name) % 2:
                raise ValueError(f"{name} must be even and >= 0")
        if self.num_wood < lanes:
            raise ValueError("num_wood must hold the 12 lane woods (or no_lanes=True)")
        if self.num_rigid // 2 + (self.num_wood - lanes) // 2 > 40:
            raise ValueError("num_rigid / 2 + (num_wood - lane woods) / 2 must be <= 40: the board has 40 free mirror pairs")
        if not 0 <= self.num_items <= self.num_wood:
            raise ValueError("num_items must be 0..num_wood")
        if not 0 <= self.max_inaccessible <= 121:
            raise ValueError("max_inaccessible must be 0..121")

    def as_tuple(self):
        return self.num_rigid, self.num_wood, self.num_items, self.max_inaccessible, self.flags

    def __repr__(self):
        return f"BoardLayout({self.num_rigid}, {self.num_wood}, {self.num_items}, {self.max_inaccessible}, no_lanes={bool(self.flags)})"


def new_games(n: int, device=None):
    """The game counters deal() reads and counts up: int32 [n] of zeros, a torch tensor on `device` (a torch device, a GPU's index, or
    None: cuda:0).  Entry e is the number of the next board env e is dealt."""
    import torch
    dev = torch.device("cuda", 0 if device is None else device) if device is None or isinstance(device, int) else torch.device(device)
    return torch.zeros((int(n),), dtype=torch.int32, device=dev)


_DEAL_MODES = {"start": DEAL_START, "next": DEAL_NEXT}
_DEAL_WHICH = {"all": DEAL_ALL, "restarted": DEAL_RESTARTED, "done": DEAL_DONE}


def move_towards(reach: dict, targets):
    """Walk to the nearest target: int32 [n, 4], per env and agent the `move` entry of the target cell with the smallest nonzero
    `dist` — ties go to the lowest cell index y * 11 + x — and 0 (IDLE) where no target is reached (a dead agent's rows reach
    nothing).  `reach`: what BatchEnvironment.reach() returns, both tensors; `targets`: bool [n, 4, 11, 11] on their device, e.g.
    the power-up cells of an observation, the same for all four agents.  Pure torch: no library call, no copy to the host."""
    import torch
    dist, move = reach["dist"], reach["move"]
    if targets.dtype != torch.bool or tuple(targets.shape) != tuple(dist.shape) or tuple(move.shape) != tuple(dist.shape):
        raise ValueError(f"targets must be bool {list(dist.shape)}, as reach's tensors are, got {targets.dtype} {list(targets.shape)}")
    d = dist.flatten(2).to(torch.int32)
    # a key per cell that orders by distance, then by cell index: no target or not reached sorts behind every real key
    key = torch.where(targets.flatten(2) & (d != 0), d * 128 + torch.arange(121, device=d.device, dtype=torch.int32), 1 << 20)
    best, cell = key.min(dim=2)
    return torch.where(best < (1 << 20), move.flatten(2).gather(2, cell.unsqueeze(2)).squeeze(2).to(torch.int32), 0)


def new_view_memory(n: int, device=None):
    """A wiped (memory, stamp) pair for BatchEnvironment.remember(): `memory` uint8 [n, 4, 6, 11, 11] with board 5 (fog), planes 1..4
    = 0 and age 255 in every cell, `stamp` int32 [n, 4, 2] of -1 ("no memory yet"); torch tensors on `device` (a torch device, a GPU's
    index, or None: cuda:0)."""
    import torch
    dev = torch.device("cuda", 0 if device is None else device) if device is None or isinstance(device, int) else torch.device(device)
    memory = torch.zeros((int(n), 4, MEMORY_PLANES, 11, 11), dtype=torch.uint8, device=dev)
    memory[:, :, 0] = 5
    memory[:, :, MEMORY_PLANES - 1] = MEMORY_AGE_NEVER
    return memory, torch.full((int(n), 4, 2), -1, dtype=torch.int32, device=dev)


def chain_litmus(tiles: int, launches: int, streams: int, device: int = 0) -> dict:
    """pom_chain_litmus: the hand-off of chained launches tested by itself (every visit checks the whole record the visit before
    left)"""
    lib = load_library()
    out = np.zeros(6, dtype=np.int64)
    _check(lib, lib.pom_chain_litmus(device, tiles, launches, streams, out.ctypes.data))
    return dict(zip(("bad_records", "bad_dwords", "visits", "visits_expected", "tiles_wrong", "flags"), (int(v) for v in out)))


def _one_state(state: np.ndarray, moves):
    """step_one's and env_step_one's arguments as the buffers the library takes"""
    assert state.dtype == STATE_DTYPE and state.size == 1
    mv = np.ascontiguousarray(moves, dtype=np.int32)
    assert mv.shape == (4,)
    return np.ascontiguousarray(state).reshape(1), mv


def step_one(state: np.ndarray, moves) -> None:
    """`bboard::Step(State*, Move*)` on one host State, executed on the GPU (pom_step)."""
    lib = load_library()
    buf, mv = _one_state(state, moves)
    _check(lib, lib.pom_step(buf.ctypes.data, mv.ctypes.data))
    state[...] = buf.reshape(state.shape)


def env_step_one(state: np.ndarray, moves, max_steps: int = 0) -> dict:
    """`Environment::Step`'s tick + bookkeeping on one host State (pom_env_step): timeStep++, done / winner / draw of this
    tick.  The caller does not step a finished game (environment.cpp:125)."""
    lib = load_library()
    buf, mv = _one_state(state, moves)
    out = np.zeros(4, dtype=np.int32)
    _check(lib, lib.pom_env_step(buf.ctypes.data, mv.ctypes.data, int(max_steps), out[0:].ctypes.data, out[1:].ctypes.data,
                                 out[2:].ctypes.data, out[3:].ctypes.data))
    state[...] = buf.reshape(state.shape)
    return {"done": int(out[0]), "winner": int(out[1]), "draw": int(out[2]), "ubflags": int(out[3]) & 0xFFFFFFFF}


class BatchEnvironment:
    def __init__(self, n_envs: int, device: int = 0, mode: int = MODE_ENV, auto_reset: bool = False,
                 max_steps: int = 0, env_offset: int = 0, stream: Optional[int] = None, envs_per_wave: int = 0,
                 streams: int = 0, lanes_per_env: int = 0, fresh_boards: bool = False, board_seed: int = 0,
                 issue_mode: int = ISSUE_AUTO):
        self._lib = load_library()
        self._h = C.c_void_p()
        self._views = []  # weak references to tensors that alias the handle's device memory (moves_tensor)
        self._tapes = []  # move tapes handed to step_device_many, kept alive until the handle has been synchronised
        self.n = int(n_envs)
        self.device = int(device)
        o = _spec(_Options, device, stream, mode, int(auto_reset), max_steps, env_offset, envs_per_wave, streams, lanes_per_env,
                  int(fresh_boards), board_seed, issue_mode, 0)
        _check(self._lib, self._lib.pom_batch_create(C.byref(self._h), self.n, C.byref(o)))

    def close(self) -> None:
        if any(r() is not None for r in getattr(self, "_views", ())):
            raise RuntimeError("close(): a tensor returned by moves_tensor() still views this handle's device memory; "
                               "delete it first")
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.pom_batch_destroy(self._h)  # waits for everything queued
            self._h = C.c_void_p()
            self._tapes = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- what the calls share --------------------------------------------------------------------------
    def _call(self, name: str, *args) -> None:
        """the library's `name` on this handle; anything but POM_OK raises PomError with the library's text"""
        rc = getattr(self._lib, name)(self._h, *args)
        if rc:
            _check(self._lib, rc)

    def _span(self, first, count):
        """(first, count) of the calls that read a range of envs: no count means all from `first` on"""
        return first, self.n - first if count is None else count

    def _in_batch(self, first, count):
        """the range [first, first + count) as ints, refused unless it lies in the batch"""
        first, count = int(first), int(count)
        if first < 0 or count < 0 or first + count > self.n:
            raise ValueError(f"the range [{first}, {first + count}) lies outside the batch of {self.n} envs")
        return first, count

    def _device_tensor(self, t, what: str, dtype, shape):
        """`t` as an argument that a kernel reads or writes through its address: anything with data_ptr / shape / dtype (e.g. a torch
        tensor) of the element type named `dtype` (such as "int32") and of `shape` (None: a free dimension), contiguous
        and on this handle's device; contiguity and device are checked where the object tells them.  Returns `t`."""
        if not hasattr(t, "data_ptr"):
            raise ValueError(f"{what} must be a device tensor {self._want(dtype, shape)}, got {type(t).__name__}")
        got = tuple(getattr(t, "shape", ()))
        if len(got) != len(shape) or any(w is not None and w != g for w, g in zip(shape, got)):
            raise ValueError(f"{what} must be {self._want(dtype, shape)}, got shape {got}")
        if _dtype_name(getattr(t, "dtype", "")) != dtype:
            raise ValueError(f"{what} must be {dtype}, got {getattr(t, 'dtype', None)}")
        if hasattr(t, "is_contiguous") and not t.is_contiguous():
            raise ValueError(f"{what} must be contiguous")
        dev = getattr(t, "device", None)
        if dev is not None and (getattr(dev, "type", "cuda") != "cuda" or getattr(dev, "index", self.device) not in (None, self.device)):
            raise ValueError(f"{what} lives on {dev}, the batch on device {self.device}")
        return t

    @staticmethod
    def _want(dtype: str, shape) -> str:
        return f"{dtype}[{', '.join('*' if w is None else str(w) for w in shape)}]"

    def _moves(self, moves, raw: bool = False, shape=None):
        """the moves argument, int32 of `shape` ([n, 4] unless given), checked; returns its address (None: NULL).  With `raw` anything
        that is no tensor is a device address the caller vouches for."""
        if moves is None:
            return None
        if raw and not hasattr(moves, "data_ptr"):
            return int(moves)
        return self._device_tensor(moves, "moves", "int32", shape or (self.n, 4)).data_ptr()

    def _torch_device(self):
        """(torch, this handle's device as torch names it)"""
        import torch
        return torch, torch.device("cuda", self.device)

    def _new(self, shape, dtype: str):
        """a new tensor of the element type named `dtype` on the handle's device: the one place a call's result is allocated"""
        torch, dev = self._torch_device()
        return torch.empty(shape, dtype=getattr(torch, dtype), device=dev)

    def _new_attrs(self, width: int, rows: int = 4):
        """new (agent_attrs or viewer_attrs, env_attrs) for an observation (`rows`: the compact views' viewers)"""
        return self._new((self.n, rows, width), "int32"), self._new((self.n, 4), "int32")

    def _out_tensor(self, out, shape, dtype, what: str = "out"):
        """the tensor a call writes its result to: a new one, or the caller's `out` of an earlier call, checked"""
        return self._new(shape, dtype) if out is None else self._device_tensor(out, what, dtype, shape)

    def _outputs(self, out, want: dict, fill=None) -> dict:
        """a call's dict of outputs, `want` = {name: (shape, dtype)}: each the tensor under that name in the caller's `out`, checked,
        or a new one (set to `fill` where that is given)"""
        res = {}
        for name, (shape, dtype) in want.items():
            given = None if out is None else out.get(name)
            res[name] = self._out_tensor(given, shape, dtype, f"out[{name!r}]")
            if given is None and fill is not None:
                res[name].fill_(fill)
        return res

    def _observation(self, codes=None, planes=None, per_agent=None, view_radius=None, viewer_attrs=None, agent_attrs=None,
                     env_attrs=None, *, raw: bool = False, dtype=None, out=None, compact=None):
        """The rules of an observation request (pom_api_observe.h's observe_args and view_args), stated once for observe(),
        step_device_observe(), step_device_range() and expand().  The layout is given as `codes` or `planes` (the element type is the
        tensor's, read by name), or as observe()'s `dtype` name with an optional `out`; with `raw` anything that is no tensor is a
        device address the caller vouches for (planes then are uint8).  Contradictions and wrong tensors are refused with a ValueError;
        no torch, no runtime call.  Returns a plain tuple, what every caller needs first (this is on the closed loop's host path, where
        a named tuple costs half a microsecond a call): (the tensor or address the planes go to — None: to be allocated, or no
        observation —, the library's dtype code, per_agent, view: these are the fogged views, the width of agent_attrs (8) or
        viewer_attrs (12) — int32 [n, 4, width], env_attrs int32 [n, 4] —, the planes' shape, their element type by name).
        `compact` (_compact_views: the viewers' mask and flags): the compact views — codes only, uint8 [n, k, 5, S, S] with S = 11 or,
        centred, 2 view_radius + 1, and viewer_attrs int32 [n, k, 12]."""
        view = view_radius is not None
        if codes is not None and planes is not None:
            raise ValueError("codes and planes are two forms of one observation: pass one")
        if dtype is None:
            out, name, is_codes = (codes, "codes", True) if codes is not None else (planes, "planes", False)
            checked = hasattr(out, "data_ptr") or (out is not None and not raw)
            dtype = "uint8" if is_codes or not checked else _dtype_name(getattr(out, "dtype", ""))
            if dtype not in _PLANE_CODES:
                raise ValueError(f"planes must be uint8, float16 or float32, got {getattr(out, 'dtype', None)}")
        else:
            name, is_codes, checked = "out", dtype == "codes", out is not None
            if not is_codes and dtype not in _PLANE_CODES:
                raise ValueError(f"dtype must be one of {sorted([*_PLANE_CODES, 'codes'])}")
            dtype = "uint8" if is_codes else dtype
        if per_agent and is_codes and not view:
            raise ValueError("the codes layout has no per-agent view (but for the fogged ones: view_radius)")
        if view and per_agent is not None and not per_agent:
            raise ValueError("view_radius gives every agent its own view: per_agent=False contradicts it")
        if view:
            _bounded(view_radius, "view_radius", 0, 10)
        if viewer_attrs is not None and not view:
            raise ValueError("viewer_attrs are written with the fogged views only: pass view_radius")
        if agent_attrs is not None and view:
            raise ValueError("agent_attrs are written with the plain observation only: the fogged views have viewer_attrs")
        per_agent, depth, width = bool(per_agent) or view, 5 if is_codes else 16, 12 if view else 8
        shape = (self.n, 4, depth, 11, 11) if per_agent else (self.n, depth, 11, 11)
        viewers = 4
        if compact is not None:
            if not view:
                raise ValueError("viewers and centred choose among the fogged views: pass view_radius")
            if not is_codes:
                raise ValueError("viewers and centred are for the codes layout only (the 16-plane views are always four, uncropped)")
            viewers, side = bin(compact[0]).count("1"), 2 * int(view_radius) + 1 if compact[1] & VIEW_CENTRED else 11
            shape = (self.n, viewers, depth, side, side)
        if checked:
            self._device_tensor(out, name, dtype, shape)
        if viewer_attrs is not None or agent_attrs is not None or env_attrs is not None:
            for t, what, want in ((viewer_attrs, "viewer_attrs", (self.n, viewers, width)), (agent_attrs, "agent_attrs", (self.n, 4, width)),
                                  (env_attrs, "env_attrs", (self.n, 4))):
                if hasattr(t, "data_ptr"):
                    self._device_tensor(t, what, "int32", want)
        return out, 3 if is_codes else _PLANE_CODES[dtype], per_agent, view, width, shape, dtype

    @contextlib.contextmanager
    def _ordered(self, back: bool = True, tensor=None):
        """The kernel runs on the handle's stream, the tensors live on torch's current stream: the two are ordered with events.  Before
        the body the handle's stream waits for torch's — a tensor the caller has just produced there is complete before the call that
        reads it begins — and, with `back`, torch's waits for the handle's after it: what the call wrote is complete before torch
        reads it.  A no-op if both are the same stream, or if `tensor` is not torch's."""
        if "torch" not in sys.modules or (tensor is not None and not hasattr(tensor, "is_cuda")):
            yield
            return
        torch, dev = self._torch_device()
        mine, theirs = torch.cuda.ExternalStream(self.stream_handle(), device=dev), torch.cuda.current_stream(dev)
        if mine.cuda_stream != theirs.cuda_stream:
            mine.wait_stream(theirs)
        yield
        if back and mine.cuda_stream != theirs.cuda_stream:
            theirs.wait_stream(mine)

    # ---- Environment::MakeGame / GetState ---------------------------------------------------
    def make_game(self, states: np.ndarray, first: int = 0) -> None:
        """Upload start states; they also become the reset snapshot (MakeGame, environment.cpp:53-66)."""
        st = np.ascontiguousarray(states, dtype=STATE_DTYPE)
        self._call("pom_batch_upload", st.ctypes.data, first, st.size)

    upload = make_game

    def generate(self, board_seed: int) -> None:
        """Start boards drawn on the device (pom_batch_generate, include/pom_boardgen.h): InitState's distribution, no host."""
        self._call("pom_batch_generate", board_seed)

    def episodes(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """games started so far per env (0 = still the first)"""
        first, count = self._span(first, count)
        out = np.zeros(count, dtype=np.uint32)
        self._call("pom_batch_episodes", first, count, out.ctypes.data)
        return out

    def get_state(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        first, count = self._span(first, count)
        out = np.zeros(count, dtype=STATE_DTYPE)
        self._call("pom_batch_download", out.ctypes.data, first, count)
        self._tapes.clear()  # the call has synchronised the handle: nothing reads a tape any more
        return out

    download = get_state

    def snapshot(self) -> None:
        self._call("pom_batch_snapshot")

    # ---- copy / restore games by index (tree search, rollouts, populations) ---------------------------
    def copy_envs(self, src, first: int = 0, *, from_snapshot: bool = False, set_snapshot: bool = False,
                  count: Optional[int] = None) -> None:
        """Env first + i becomes a copy of env src[i] (pom_batch_copy_envs): record, SimpleAgent memory, episode counter and, with
        RESET_AT_END, the last finished episode — as if every source were read before any destination is written (sources may lie
        in the range and repeat).  Entries < 0 leave their env alone.  from_snapshot: copy src[i]'s restart snapshot instead (fresh
        agents; episode and terminal record stay).  set_snapshot: the copy also becomes the destination's snapshot.
        src: a numpy integer array (host variant: entries >= n raise), a torch int64 tensor on this handle's device (device variant,
        read in stream order behind torch's current stream; entries >= n are left alone too), or a raw device address of int64
        with `count`."""
        flags = (COPY_FROM_SNAPSHOT if from_snapshot else 0) | (COPY_SET_SNAPSHOT if set_snapshot else 0)
        if hasattr(src, "data_ptr"):
            self._device_tensor(src, "src", "int64", (count,))
            with self._ordered(back=False, tensor=src):
                self._call("pom_batch_copy_envs_device", src.data_ptr(), int(first), src.shape[0], flags)
        elif isinstance(src, (int, np.integer)) and not isinstance(src, bool):
            if count is None:
                raise ValueError("a raw device address needs `count`")
            self._call("pom_batch_copy_envs_device", int(src), int(first), int(count), flags)
        else:
            idx = np.asarray(src)
            if idx.ndim != 1 or not np.issubdtype(idx.dtype, np.integer):
                raise ValueError("src must be a 1-d integer array")
            idx = np.ascontiguousarray(idx, dtype=np.int64)
            if count is not None and count != idx.size:
                raise ValueError(f"count {count} does not match src of {idx.size} entries")
            self._call("pom_batch_copy_envs", idx.ctypes.data, int(first), idx.size, flags)

    def restore(self, envs) -> None:
        """Put the given envs back on their restart snapshot with fresh agents: a boolean mask of n, or a list of env indices.
        A thin wrapper over copy_envs(..., from_snapshot=True)."""
        envs = np.asarray(envs)
        if envs.dtype == bool:
            if envs.shape != (self.n,):
                raise ValueError(f"a mask must have {self.n} entries, got {envs.shape}")
            src = np.where(envs, np.arange(self.n, dtype=np.int64), -1)
            self.copy_envs(src, 0, from_snapshot=True)
            return
        idx = np.unique(np.ascontiguousarray(envs, dtype=np.int64).reshape(-1))
        if idx.size == 0:
            return
        if idx[0] < 0 or idx[-1] >= self.n:
            raise ValueError(f"env indices must lie in [0, {self.n})")
        lo, hi = int(idx[0]), int(idx[-1]) + 1
        src = np.full(hi - lo, -1, dtype=np.int64)
        src[idx - lo] = idx
        self.copy_envs(src, lo, from_snapshot=True)

    # ---- Environment::Step --------------------------------------------------------------------
    def step(self, moves: np.ndarray) -> None:
        mv = np.ascontiguousarray(moves, dtype=np.int32)
        if mv.shape != (self.n, 4):
            raise ValueError(f"moves must be int32[{self.n}, 4] (dead agents included), got {mv.shape}")
        self._call("pom_batch_step", mv.ctypes.data)

    def step_device(self, moves) -> None:
        """moves: a device tensor int32[n,4] on this handle's device (anything with data_ptr / shape / dtype, e.g. a torch
        tensor: shape, element type, contiguity and device are checked), or the raw device address of such an array."""
        ptr = self._moves(moves, raw=True)
        with self._ordered(back=False, tensor=moves):
            self._call("pom_batch_step_device", ptr)

    def step_device_many(self, moves, ticks: Optional[int] = None) -> None:
        """K ticks with explicit moves from a tape in device memory: a tensor int32[K, n, 4] on this handle's device (or the raw
        device address of one, with `ticks` = K).  Chained launches where the handle chains (pom_batch_step_device_many)."""
        ptr = self._moves(moves, raw=True, shape=(ticks, self.n, 4))
        if hasattr(moves, "data_ptr"):
            ticks = moves.shape[0]
            # the tape is read asynchronously and must stay unchanged until the handle has been synchronised: keep the tensor (and
            # with it its memory) alive until then, whatever the caller does with its own reference
            if len(self._tapes) >= 4:  # a loop that never synchronises must not keep every tape alive: wait for the old ones
                self.sync()
            self._tapes.append(moves)
        if ticks is None:
            raise ValueError("a raw device address needs `ticks`")
        with self._ordered(back=False, tensor=moves):
            self._call("pom_batch_step_device_many", ptr, int(ticks))

    def step_device_range(self, first: int, count: int, moves, stream=None, codes=None, planes=None, view_radius: Optional[int] = None,
                          viewer_attrs=None, env_attrs=None, *, per_agent: Optional[bool] = None, agent_attrs=None) -> None:
        """Closed-loop stepping (pom_batch_step_device_range): one tick for the envs [first, first + count) — whole tiles of 16 — as ONE
        launch on `stream` (a raw hipStream_t / torch stream; None: the handle's stream), Move[4] from `moves` (int32[n, 4] device tensor
        or address, indexed by env).  `codes` (uint8[n, 5, 11, 11]) or `planes` ([n, 16, 11, 11] or, with `per_agent`, [n, 4, 16, 11, 11] of
        uint8 / float16 / float32, the element type is the tensor's): the observation of those envs after the tick, written by the same
        launch, and with it optionally `agent_attrs` int32[n, 4, 8] and `env_attrs` int32[n, 4].  Every array is sized for the WHOLE batch
        and indexed by env; only the range's rows are written.  Nothing is forked or joined: the stream orders the call; sync() the handle
        once before a loop of these (and before capturing them into a graph).  `view_radius`: the four agents' fogged views instead
        (pom_batch_step_device_range_view) — `codes` uint8[n, 4, 5, 11, 11] or `planes` [n, 4, 16, 11, 11] of uint8 / float16 / float32, and
        optionally `viewer_attrs` int32[n, 4, 12] and `env_attrs` int32[n, 4].
        Every tensor (anything with data_ptr / shape / dtype) is checked — element type, shape, contiguity, device — and a range outside
        the batch, `codes` together with `planes`, `per_agent` with `codes` and attribute arrays that nothing would write are refused,
        all with a ValueError before anything is launched; a raw device address passes unchecked (planes then are uint8).  The checks
        make no runtime call."""
        first, count = self._in_batch(first, count)
        out, code, per_agent, view, _width, _shape, _dtype = self._observation(codes, planes, per_agent, view_radius, viewer_attrs, agent_attrs,
                                                                                env_attrs, raw=True)
        if out is None and (per_agent or agent_attrs is not None or env_attrs is not None):
            raise ValueError("view_radius, per_agent, agent_attrs and env_attrs belong to an observation: pass `codes` or `planes`")
        ptr, st = self._moves(moves, raw=True), getattr(stream, "cuda_stream", stream)
        if view:
            spec = _view_spec(code, view_radius, out, viewer_attrs, env_attrs)
            self._call("pom_batch_step_device_range_view", first, count, ptr, st, C.byref(spec))
        else:
            self._call("pom_batch_step_device_range", first, count, ptr, st, _ptr(out), code, int(per_agent), _ptr(agent_attrs), _ptr(env_attrs))

    def _mixed_step_spec(self, first, count, moves, simple, seed, tick, stream, codes, planes, view_radius, viewer_attrs, env_attrs, per_agent,
                         agent_attrs, viewers=None, centred=False) -> _MixedStepSpec:
        """step_mixed()'s arguments checked, as the PomMixedStepSpec that step_mixed() and step_events() hand to the library"""
        first, count = self._in_batch(first, count)
        mask, tick, compact = _agent_mask(simple, "simple"), _bounded(tick, "tick", 0, 0xFFFFFFFF), _compact_views(viewers, centred)
        out, code, per_agent, view, _width, _shape, _dtype = self._observation(codes, planes, per_agent, view_radius, viewer_attrs, agent_attrs,
                                                                                env_attrs, raw=True, compact=compact)
        if out is None and (per_agent or agent_attrs is not None or env_attrs is not None):
            raise ValueError("view_radius, per_agent, agent_attrs and env_attrs belong to an observation: pass `codes` or `planes`")
        if moves is None and mask != 15:
            raise ValueError("moves is None, but simple leaves agents to it")
        ptr, st = self._moves(moves, raw=True), getattr(stream, "cuda_stream", stream)
        if view:
            vs = _view_spec(code, view_radius, out, viewer_attrs, env_attrs, compact)
            spec = _spec(_MixedStepSpec, mask, first, count, ptr, _u64(seed), tick, st, C.pointer(vs), None, 0, 0, None, None, 0, 0)
        else:
            spec = _spec(_MixedStepSpec, mask, first, count, ptr, _u64(seed), tick, st, None, _ptr(out), code if out is not None else 0,
                         int(per_agent), _ptr(agent_attrs), _ptr(env_attrs), 0, 0)
        return spec

    def step_mixed(self, first: int, count: int, moves, simple, seed: int, tick: int, stream=None, codes=None, planes=None,
                   view_radius: Optional[int] = None, viewer_attrs=None, env_attrs=None, *, per_agent: Optional[bool] = None,
                   agent_attrs=None, viewers=None, centred: bool = False) -> None:
        """step_device_range() with SimpleAgent opponents (pom_batch_step_mixed): one tick for the envs [first, first + count) — whole
        tiles of 16 — as ONE launch on `stream`, in which the agents of `simple` (a mask int 0..15 or an iterable of agent ids) are
        played by SimpleAgent inside the launch — asked as policy_simple(seed) asks them at handle tick `tick` (0..2^32-1), their memory
        (policy_memory()) moved on — and the others take `moves[e][a]` (int32[n, 4] device tensor or address, indexed by env; None only
        if all four agents are SimpleAgents).  The ranges of a closed loop advance on their own, so the caller counts each range's
        `tick`; the handle's tick, its move buffer and the envs outside the range are left alone.  The observation arguments, the
        checks (a ValueError before anything is launched, no runtime call) and the ordering are step_device_range()'s.  The first call
        with a non-empty `simple` on a handle that has run no policy yet allocates the agents' memory and synchronises the handle's
        stream once: make it — count 0 does only that — before capturing mixed steps into a graph.
        `viewers` (a mask int or an iterable of agent ids) and `centred`, with `view_radius` and `codes`: the compact views
        (PomCompactViewSpec) — only those k agents' views, `codes` uint8[n, k, 5, 11, 11], or centred each cropped to its window,
        uint8[n, k, 5, S, S] with S = 2 view_radius + 1 (fog = off the board), and `viewer_attrs` int32[n, k, 12].  A single learner
        reads `viewers=[0], centred=True`: a sixth of the four views' bytes, already a dense batch."""
        self._call("pom_batch_step_mixed", C.byref(self._mixed_step_spec(first, count, moves, simple, seed, tick, stream, codes, planes, view_radius,
                                                                         viewer_attrs, env_attrs, per_agent, agent_attrs, viewers, centred)))

    def _events_tensor(self, t, what: str, dtypes, shape):
        """an array step_events() writes: a device tensor of one of the element types named in `dtypes` and of `shape`, or a raw
        device address the caller vouches for; returns its address (None: NULL)"""
        if t is None or not hasattr(t, "data_ptr"):
            return None if t is None else int(t)
        name = _dtype_name(getattr(t, "dtype", ""))
        return self._device_tensor(t, what, name if name in dtypes else dtypes[0], shape).data_ptr()

    def step_events(self, first: int, count: int, moves, simple, seed: int, tick: int, events, outcome=None, wood=None, stream=None,
                    codes=None, planes=None, view_radius: Optional[int] = None, viewer_attrs=None, env_attrs=None, *,
                    per_agent: Optional[bool] = None, agent_attrs=None, viewers=None, centred: bool = False) -> None:
        """step_mixed() that also says what the tick did (pom_batch_step_events; the rule is PomStepEventsSpec's in include/pom_batch.h):
        the same ONE launch on `stream`, everything step_mixed() leaves bit for bit, and for the envs of the range `events` — uint32 or
        int32 [n, 4], one word per agent: the move it played (a SimpleAgent's included), whether it died, moved, laid a bomb, gained a
        power-up, how many of its bombs went off, and whether the tick ended the episode and how (decode_step_events(); the EV_*
        constants) —, `outcome` (optional, uint32 or int32 [n]: decode_rollout()'s word of the state the tick left BEFORE a restart at
        the end — on an END tick under RESET_AT_END what last_results() reports, without the host) and `wood` (optional, uint8 [n]: wood
        cells burnt by this tick).  The arrays are sized for the whole batch and indexed by env, as `moves` is; rows outside the range are
        not touched.  Every other argument, check and ordering rule is step_mixed()'s; no runtime call is made here."""
        spec = self._mixed_step_spec(first, count, moves, simple, seed, tick, stream, codes, planes, view_radius, viewer_attrs, env_attrs,
                                     per_agent, agent_attrs, viewers, centred)
        if events is None:
            raise ValueError("events is None: step_events() writes the event words there (step_mixed() is the call without them)")
        ev = _spec(_StepEventsSpec, 0, self._events_tensor(events, "events", ("uint32", "int32"), (self.n, 4)),
                   self._events_tensor(outcome, "outcome", ("uint32", "int32"), (self.n,)),
                   self._events_tensor(wood, "wood", ("uint8",), (self.n,)), 0)
        self._call("pom_batch_step_events", C.byref(spec), C.byref(ev))

    def chain_stats(self) -> dict:
        """chained launches since creation: launches issued, checks run, tiles found left behind, ticks replayed for them"""
        out = np.zeros(4, dtype=np.int64)
        self._call("pom_batch_chain_stats", out.ctypes.data)
        return dict(zip(("launches", "settles", "tiles_recovered", "ticks_replayed"), (int(v) for v in out)))

    def step_random(self, seed: int, dist: int = DIST_RANDOM, ticks: int = 1, ticks_per_launch: int = 1) -> None:
        self._call("pom_batch_step_random", seed, dist, ticks, ticks_per_launch)

    # ---- SimpleAgent policy on the device (agents::SimpleAgent) -------------------------------------
    def policy_simple(self, seed: int, want_moves: bool = False):
        """act() of all four agents of every env into the internal move buffer; optionally returns int32[n,4]."""
        out = np.zeros((self.n, 4), dtype=np.int32) if want_moves else None
        self._call("pom_batch_policy_simple", seed, out.ctypes.data if want_moves else None)
        return out

    def step_policy(self) -> None:
        self._call("pom_batch_step_policy")

    def step_simple(self, seed: int, ticks: int = 1) -> None:
        self._call("pom_batch_step_simple", seed, ticks)

    def policy_memory(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        first, count = self._span(first, count)
        out = np.zeros((count, 4, 16), dtype=np.int32)
        self._call("pom_batch_policy_memory", first, count, out.ctypes.data)
        return out

    def set_tick(self, tick: int) -> None:
        self._call("pom_batch_set_tick", tick)

    # ---- IsDone / IsDraw / GetWinner ------------------------------------------------------------
    def _int32_columns(self, name: str, names, first, count) -> dict:
        """the library's `name` read into one int32[count] array per entry of `names`"""
        first, count = self._span(first, count)
        arrs = [np.zeros(count, dtype=np.int32) for _ in names]
        self._call(name, first, count, *[a.ctypes.data for a in arrs])
        return dict(zip(names, arrs))

    def status(self, first: int = 0, count: Optional[int] = None) -> dict:
        out = self._int32_columns("pom_batch_status", ("done", "winner", "draw", "alive", "time_step", "ubflags"), first, count)
        self._tapes.clear()
        out["ubflags"] = out["ubflags"].view(np.uint32)
        return out

    def last_results(self, first: int = 0, count: Optional[int] = None) -> dict:
        """auto_reset=RESET_AT_END: `finished` = the env's latest tick ended an episode (it now stands on its next start state);
        winner / draw / length / alive describe the env's most recently finished episode."""
        return self._int32_columns("pom_batch_last_results", ("finished", "winner", "draw", "length", "alive"), first, count)

    def get_terminal_state(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """auto_reset=RESET_AT_END: the final State of each env's most recently finished episode (zeros: none yet)"""
        first, count = self._span(first, count)
        out = np.zeros(count, dtype=STATE_DTYPE)
        self._call("pom_batch_download_terminal", out.ctypes.data, first, count)
        return out

    def is_done(self) -> np.ndarray:
        return self.status()["done"].astype(bool)

    def is_draw(self) -> np.ndarray:
        return self.status()["draw"].astype(bool)

    def get_winner(self) -> np.ndarray:
        return self.status()["winner"]

    # ---- observation export ---------------------------------------------------------
    def step_device_observe(self, moves, per_agent: Optional[bool] = None, dtype: str = "uint8", attrs: bool = True, out=None,
                            view_radius: Optional[int] = None):
        """step_device(moves) and observe(...) as ONE launch (pom_batch_step_device_observe / _view): returns what observe() would."""
        return self.observe(per_agent=per_agent, dtype=dtype, attrs=attrs, out=out, view_radius=view_radius, _step_moves=moves)

    def observe(self, per_agent: Optional[bool] = None, dtype: str = "uint8", attrs: bool = True, out=None,
                view_radius: Optional[int] = None, _step_moves=None, *, viewers=None, centred: bool = False):
        """Planes of every env as torch tensors on the handle's device, written by one kernel on the handle's stream
        (pom_batch_observe; plane list in include/pom_batch.h).  Returns (planes, agent_attrs, env_attrs): planes
        [n,16,11,11] or [n,4,16,11,11]; agent_attrs int32 [n,4,8]; env_attrs int32 [n,4] (None, None if attrs=False).
        dtype "codes": the compact form, uint8 [n,5,11,11] = board codes 0..13, bomb strength / life / direction, flame life
        (POM_OBS_CODES; no per-agent view).  `out` reuses a planes tensor from an earlier call.  torch is only the owner of the
        device memory here.
        view_radius (0..10; 4 = Pommerman's 9x9 window): partial observability (pom_batch_observe_view) — every agent's view through
        the window around itself, fog elsewhere.  Returns (planes, viewer_attrs, env_attrs): planes [n,4,16,11,11], all-zero cells
        outside the window, or for "codes" [n,4,5,11,11] with board code 5 (fog) outside it; viewer_attrs int32 [n,4,12] = the
        viewer's own agent_attrs row, the alive flags of the next three agents, the time step.  per_agent is implied.
        `viewers` (a mask int or an iterable of agent ids) and `centred`, with view_radius and dtype "codes": the compact views
        (PomCompactViewSpec) — only those k agents' views, planes [n,k,5,11,11], or centred each cropped to its window: [n,k,5,S,S],
        S = 2 view_radius + 1, byte [dy][dx] the cell (x_v - r + dx, y_v - r + dy), code 5 off the board; viewer_attrs [n,k,12]."""
        compact = _compact_views(viewers, centred)
        if compact is not None and _step_moves is not None:
            raise ValueError("step_device_observe() has no compact views: step_mixed() with simple=0 is the fused call that serves them")
        out, code, per_agent, view, width, shape, elem = self._observation(per_agent=per_agent, view_radius=view_radius, dtype=dtype, out=out,
                                                                            compact=compact)
        if out is None:
            out = self._new(shape, elem)
        a_attrs, e_attrs = self._new_attrs(width, shape[1] if compact else 4) if attrs else (None, None)
        step = () if _step_moves is None else (self._moves(_step_moves),)
        name = "pom_batch_observe" if _step_moves is None else "pom_batch_step_device_observe"
        with self._ordered():
            if view:
                self._call(name + "_view", *step, C.byref(_view_spec(code, view_radius, out, a_attrs, e_attrs, compact)))
            else:
                self._call(name, *step, out.data_ptr(), code, int(per_agent), _ptr(a_attrs), _ptr(e_attrs))
        return out, a_attrs, e_attrs

    # ---- forecast: flames and deaths K ticks ahead (pom_batch_forecast) ---------------------------------
    def forecast(self, horizon: int, moves=None, out=None, agent_ticks: bool = True, ubflags: bool = False) -> dict:
        """Where will the fire be, and when: `horizon` (1..32) ticks of bboard::Step played on a scratch copy of every env by one
        kernel on the handle's stream; the batch itself is left exactly as it is (pom_batch_forecast, include/pom_batch.h).
        `moves`: a device int32 tensor [n, 4], the moves of forecast tick 1 (None: IDLE); the later ticks are all-IDLE.
        Returns a dict of torch tensors on the handle's device: `flame_tick` uint8 [n, 11, 11], per cell the first tick 1..horizon
        that leaves it in flames (0: none); with agent_ticks `agent_tick` int32 [n, 4] (-1 dead already, t the tick the agent dies
        in, 0 alive at the end); with ubflags `ubflags` (int32 [n] holding the header's uint32 bit mask of the POM_UB_* flags the
        forecast ticks raised: test bits, do not compare signed values).  `out`: a dict
        with tensors of an earlier call under the same names, written in place of new ones."""
        horizon = _lookahead(horizon)
        want = {"flame_tick": ((self.n, 11, 11), "uint8")}
        if agent_ticks:
            want["agent_tick"] = ((self.n, 4), "int32")
        if ubflags:
            want["ubflags"] = ((self.n,), "int32")
        res = self._outputs(out, want)
        self._moves(moves)
        with self._ordered():
            self._call("pom_batch_forecast", C.byref(_forecast_spec(horizon, moves, res["flame_tick"], res.get("agent_tick"), res.get("ubflags"))))
        return res

    # ---- move safety: every agent's six moves judged in one launch (pom_batch_move_safety) ------------------
    def move_safety(self, horizon: int, agents=None, moves=None, out=None, death: bool = True, escape: bool = True) -> dict:
        """An action mask's raw material: each of the six moves (IDLE, UP, DOWN, LEFT, RIGHT, BOMB) of every agent of `agents` (a mask
        int 1..15 or an iterable of agent ids; None: all four) played as tick 1, then `horizon` - 1 (horizon 1..32) ticks standing
        still, on a scratch copy of every env by one kernel on the handle's stream; the batch itself is left exactly as it is
        (pom_batch_move_safety, include/pom_batch.h).  `moves`: a device int32 tensor [n, 4], the OTHER agents' moves of tick 1 (an
        agent's own entry is replaced by its candidate; None: IDLE).  Returns a dict of int8 [n, 4, 6] tensors on the handle's device:
        with `death` `death_tick` (-1 dead already, t the tick the agent dies in if it stands still after the move, 0 alive at the
        end — forecast()'s agent_tick for those moves), with `escape` `escape_tick` (-1 dead already, t the first tick after which a
        walker that started with the move has no free cell left to stand on, 0 there still is one when the horizon ends: the header
        defines it exactly).  `out`: a dict with tensors of an earlier call under the same names, written in place of new ones.  The
        rows of agents not asked for are -1 in a tensor this call allocates and left as they were in a caller's."""
        horizon = _lookahead(horizon)
        mask = 0xF if agents is None else _agent_mask(agents, "agents")
        if mask == 0:
            raise ValueError("agents names nobody")
        want = {name: ((self.n, 4, 6), "int8") for name, wanted in (("death_tick", death), ("escape_tick", escape)) if wanted}
        if not want:
            raise ValueError("death and escape are both False: nothing to compute")
        res = self._outputs(out, want, fill=None if mask == 0xF else -1)
        self._moves(moves)
        with self._ordered():
            spec = _spec(_MoveSafetySpec, horizon, mask, 0, _ptr(moves), _ptr(res.get("death_tick")), _ptr(res.get("escape_tick")), 0)
            self._call("pom_batch_move_safety", C.byref(spec))
        return res

    def safe_moves(self, horizon: int, agents=None, moves=None):
        """The action mask: bool [n, 4, 6], True where move_safety()'s escape_tick is 0 — the agent is alive and, having made the
        move, still has somewhere to be when the horizon ends.  Rows of dead agents and of agents not asked for are all False."""
        return self.move_safety(horizon, agents, moves, death=False)["escape_tick"] == 0

    # ---- reach: every agent's FillRMap distances and first moves in one launch (pom_batch_reach) --------------
    def reach(self, agents=None, max_dist: int = REACH_MAX_DIST, out=None, dist: bool = True, move: bool = True) -> dict:
        """Where can an agent walk, how far is it, and which way does it start: the reference's reachability map (strategy::FillRMap
        and MoveTowardsPosition) of every agent of `agents` (a mask int 1..15 or an iterable of agent ids; None: all four) in every
        env by one kernel on the handle's stream; the batch itself is left exactly as it is (pom_batch_reach, include/pom_batch.h).
        Returns a dict of uint8 [n, 4, 11, 11] tensors on the handle's device, indexed [env, agent, y, x]: with `dist` `dist`, the
        walking distance from the agent's cell (0: the agent's own cell, a cell it cannot reach, or one farther than `max_dist`,
        1..120), with `move` `move`, the first step of the reference's path to the cell (1 UP, 2 DOWN, 3 LEFT, 4 RIGHT; 0 where
        dist is 0).  A dead agent's rows are 0.  `out`: a dict with tensors of an earlier call under the same names, written in
        place of new ones.  The rows of agents not asked for are 0 in a tensor this call allocates and left as they were in a
        caller's.  move_towards(reach, targets) picks the step to the nearest of a set of cells."""
        max_dist = _bounded(max_dist, "max_dist", 1, REACH_MAX_DIST)
        mask = 0xF if agents is None else _agent_mask(agents, "agents")
        if mask == 0:
            raise ValueError("agents names nobody")
        want = {name: ((self.n, 4, 11, 11), "uint8") for name, wanted in (("dist", dist), ("move", move)) if wanted}
        if not want:
            raise ValueError("dist and move are both False: nothing to compute")
        res = self._outputs(out, want, fill=None if mask == 0xF else 0)
        with self._ordered():
            self._call("pom_batch_reach", C.byref(_spec(_ReachSpec, mask, max_dist, 0, _ptr(res.get("dist")), _ptr(res.get("move")), 0)))
        return res

    # ---- view memory: the fogged views merged into what each agent remembers (pom_batch_remember_view) ------------
    def remember(self, memory, stamp, view_radius: int = 4, agents=None, first: int = 0, count: Optional[int] = None, stream=None,
                 viewer_attrs=None, env_attrs=None) -> None:
        """What each agent saw last and how long ago (pom_batch_remember_view; include/pom_batch.h states THE RULE): the fogged views of
        the agents of `agents` (a mask int 1..15 or an iterable of agent ids; None: all four) of the envs [first, first + count) —
        whole tiles of 16; no count: all from `first` on — merged into `memory`, uint8 [n, 4, 6, 11, 11] (planes 0..4 the code bytes of
        observe(dtype="codes"), plane 5 the age: 0 seen now, 1..254 ticks ago, 255 never), as ONE launch on `stream` (a raw
        hipStream_t / torch stream; None: the handle's stream), in place of the view export of a closed loop: step_device_range() or
        step_mixed() without an observation, then this on the same stream.  Cells inside a viewer's window (`view_radius` 0..10) are
        copied with age 0; outside it remembered bombs and flames count down, agents seen elsewhere or dead are cleared and the age
        grows.  `stamp`, int32 [n, 4, 2], holds each view's (episode, timeStep) of its last update: a new game, a restore() or a
        stamp of -1 wipes the view first.  new_view_memory(n) makes a wiped pair; after copy_envs() / expand() / make_game() onto an
        env set its stamp rows to -1.  Optionally `viewer_attrs` int32 [n, 4, 12] and `env_attrs` int32 [n, 4], as observe(view_radius=)
        returns them.  Every array is sized for the WHOLE batch; only the range's rows of the mask's views are written.  The batch is
        left exactly as it is.  The tensors are checked as step_device_range() checks its own — a ValueError before anything is
        launched, no runtime call; a raw device address passes unchecked — and nothing is forked or joined: the stream orders the call."""
        first, count = self._in_batch(*self._span(int(first), count))
        view_radius = _bounded(view_radius, "view_radius", 0, 10)
        mask = 0xF if agents is None else _agent_mask(agents, "agents")
        if mask == 0:
            raise ValueError("agents names nobody")
        for t, what, dtype, shape in ((memory, "memory", "uint8", (self.n, 4, MEMORY_PLANES, 11, 11)), (stamp, "stamp", "int32", (self.n, 4, 2)),
                                      (viewer_attrs, "viewer_attrs", "int32", (self.n, 4, 12)), (env_attrs, "env_attrs", "int32", (self.n, 4))):
            if hasattr(t, "data_ptr"):
                self._device_tensor(t, what, dtype, shape)
            elif t is None and what in ("memory", "stamp"):
                raise ValueError(f"{what} must be a device tensor {self._want(dtype, shape)} or a device address, got None")
        spec = _spec(_MemorySpec, view_radius, mask, 0, _ptr(memory), _ptr(stamp), _ptr(viewer_attrs), _ptr(env_attrs))
        self._call("pom_batch_remember_view", first, count, C.byref(spec), getattr(stream, "cuda_stream", stream))

    # ---- imagine: playable games from an agent's view memory (pom_batch_imagine) ----------------------------
    def imagine(self, memory, viewer_attrs, view, first: int = 0, sample=None, seed: int = 0, unknown: str = "sample", belief=None,
                out=None, stream=None):
        """Determinization, for search under fog without peeking (pom_batch_imagine; include/pom_batch.h states THE RULE): env
        `first + j` becomes a playable game built from row `view[j]` = e * 4 + v of `memory` (uint8 [m, 4, 6, 11, 11], what remember()
        maintains — of this batch or any other) and `viewer_attrs` (int32 [m, 4, 12], as remember() or observe(view_radius=) write them),
        with sample number `sample[j]` (None: j) and `seed` keying every draw for what the viewer never saw: the same (view, sample)
        builds the same game in any slot.  `view`, `sample`: int32 [count] device tensors (or numpy arrays, which are copied there);
        a view < 0 or >= 4 m is "no job".  `unknown`: "sample" draws a never-seen cell from the start board's distribution, "passage"
        makes it passage.  `belief`: None, or int32 [m, 4, 4, 3], (maxBombCount, bombStrength, canKick) of agent a as viewer v believes
        them.  Returns the result words, int32 [count] on the handle's device holding the header's uint32 words (decode_imagine names
        the fields); `out`: such a tensor of an earlier call.  A built env is left as make_game() leaves one — status clear, the record
        also its restart snapshot, fresh SimpleAgent memory; episode counters, counters and the handle's tick are untouched — and is
        meant for the calls that never restart a game: forecast(), the rollouts, expand(), move_safety(), reach().  ONE launch on
        `stream` (a raw hipStream_t / torch stream; None: the handle's stream, ordered with torch's current one)."""
        def device_tensor(a, what, shape):  # numpy arrays are copied to the device, anything else is _device_tensor's
            if isinstance(a, np.ndarray):
                if not np.issubdtype(a.dtype, np.integer):
                    raise ValueError(f"{what} must be an integer array")
                torch, dev = self._torch_device()
                a = torch.from_numpy(np.ascontiguousarray(a, dtype="int32")).to(dev)
            return self._device_tensor(a, what, "int32", shape)

        if unknown not in ("sample", "passage"):
            raise ValueError('unknown must be "sample" or "passage"')
        view = device_tensor(view, "view", (None,))
        count = int(view.shape[0])
        first, _ = self._in_batch(first, count)
        if sample is not None:
            sample = device_tensor(sample, "sample", (count,))
        memory = self._device_tensor(memory, "memory", "uint8", (None, 4, MEMORY_PLANES, 11, 11))
        m = int(memory.shape[0])
        self._device_tensor(viewer_attrs, "viewer_attrs", "int32", (m, 4, 12))
        if belief is not None:
            self._device_tensor(belief, "belief", "int32", (m, 4, 4, 3))
        if m == 0 and count:
            raise ValueError("memory holds no view")
        out = self._out_tensor(out, (count,), "int32")
        raw = getattr(stream, "cuda_stream", stream)
        spec = _spec(_ImagineSpec, IMAGINE_SAMPLE if unknown == "sample" else IMAGINE_PASSAGE, first, count, 4 * max(m, 1), 0, _u64(seed),
                     *_job_ptrs(count, view, sample, memory, viewer_attrs, belief, out), raw)
        if raw is None:
            with self._ordered():
                self._call("pom_batch_imagine", C.byref(spec))
        else:
            self._call("pom_batch_imagine", C.byref(spec))
        return out

    # ---- deal: Pommerman's standard start boards drawn on the device (pom_batch_deal) ------------------------
    def deal(self, games, seed: int = 0, mode: str = "start", which="all", first: int = 0, count: Optional[int] = None, layout=None,
             out=None, stream=None):
        """Pommerman's standard start board — mirror-symmetric, 36 rigid walls, 36 woods, 20 hidden items, every agent one cell in from
        its corner, lanes of wood between neighbours, rejected if too many passages are walled off — for the envs [first, first + count)
        (any range; no count: all from `first` on), drawn on the device as ONE launch (pom_batch_deal; include/pom_batch.h states THE
        RULE).  generate() and fresh_boards give the reference's board instead.  `games`: int32 [n] device tensor (new_games(n)), by
        env: a dealt env e gets board (seed, env_offset + e, games[e]) and games[e] goes up by one.  `which`: "all", "restarted" (the
        envs the last tick restarted; RESET_AT_END handles), "done" (the finished ones), or an int32 [n] device tensor: the envs with a
        nonzero entry.  `mode`: "start" — the board is the env's state and its restart snapshot, status clear, fresh SimpleAgent memory
        — or "next" — it is the restart snapshot only: the board the env's next restart lands on; deal(games, seed, "next",
        "restarted") after every tick of a closed loop gives every game a new board.  `layout`: a BoardLayout (None: the standard one).
        `out`: None, or an int32 [n] device tensor for the result words, by env (decode_deal names the fields; envs of the range that
        are not dealt get 0, envs outside it are not written); returned.  `stream`: a raw hipStream_t / torch stream; None: the
        handle's stream, ordered with torch's current one.  The tensors are checked as step_device_range() checks its own — a
        ValueError before anything is launched, no runtime call."""
        if mode not in _DEAL_MODES:
            raise ValueError('mode must be "start" or "next"')
        mask = None
        if isinstance(which, str):
            if which not in _DEAL_WHICH:
                raise ValueError('which must be "all", "restarted", "done" or a mask tensor')
            which_code = _DEAL_WHICH[which]
        else:
            mask, which_code = self._device_tensor(which, "which", "int32", (self.n,)), DEAL_MASK
        first, count = self._in_batch(*self._span(int(first), count))
        self._device_tensor(games, "games", "int32", (self.n,))
        if layout is None:
            layout = BoardLayout()
        elif not isinstance(layout, BoardLayout):
            raise ValueError(f"layout must be a BoardLayout, got {type(layout).__name__}")
        if out is not None:
            self._device_tensor(out, "out", "int32", (self.n,))
        raw = getattr(stream, "cuda_stream", stream)
        spec = _spec(_DealSpec, _DEAL_MODES[mode], which_code, 0, first, count, _u64(seed), _BoardLayout(*layout.as_tuple()), 0,
                     *_job_ptrs(count, games, mask, out), raw)
        if raw is None:
            with self._ordered():
                self._call("pom_batch_deal", C.byref(spec))
        else:
            self._call("pom_batch_deal", C.byref(spec))
        return out

    # ---- rollout: R random playouts of every env (pom_batch_rollout) ---------------------------------------
    def rollout(self, horizon: int, samples: int, seed: int, dist: int = DIST_RANDOM, moves=None, out=None, *, simple=None, first=None,
                fresh_agents: bool = False):
        """How does the game end: `samples` (1..256) random playouts of every env under the move stream `dist`, each to a finished game
        or `horizon` (1..1024) ticks, by one kernel on the handle's stream; the batch itself is left exactly as it is
        (pom_batch_rollout, include/pom_batch.h).  Sample r is seeded pom_splitmix64(seed + r).  `moves`: a device int32 tensor
        [n, 4], the moves of tick 1 of every sample (None: drawn like the others).  Returns the result words, an int32 tensor
        [samples, n] on the handle's device holding the header's uint32 words (decode_rollout names the fields: test bits, do not
        compare signed values).  `out`: such a tensor of an earlier call, written in place of a new one.

        With `simple`, `first` or `fresh_agents` given the playouts are pom_batch_rollout_policy's: `simple` (a mask int 0..15 or an
        iterable of agent ids) names the agents that play SimpleAgent, starting from a copy per sample of the memory policy_memory()
        reports (`fresh_agents`: from new agents); the others draw from `dist`.  `first` (likewise) names the agents whose move of
        tick 1 is `moves[e][a]`; with `moves` given and `first` not, all four are."""
        with_policy = simple is not None or first is not None or bool(fresh_agents)
        horizon, samples, dist, simple_mask, first_mask, flags = _rollout_args(horizon, samples, dist, moves, simple, first, fresh_agents, with_policy)
        out = self._out_tensor(out, (samples, self.n), "int32")
        common = horizon, samples, dist, _u64(seed), self._moves(moves), out.data_ptr()
        with self._ordered():
            if with_policy:
                self._call("pom_batch_rollout_policy", C.byref(_spec(_RolloutPolicySpec, *common, simple_mask, first_mask, flags, 0)))
            else:
                self._call("pom_batch_rollout", C.byref(_spec(_RolloutSpec, *common, 0)))
        return out

    # ---- rollout of a list of jobs (pom_batch_rollout_jobs) ----------------------------------------------
    def rollout_jobs(self, src, horizon: int, samples: int, seed: int, dist: int = DIST_RANDOM, moves=None, out=None, *, simple=None,
                     first=None, fresh_agents: bool = False):
        """rollout()'s playouts for a list of jobs instead of every env: job j plays env `src[j]` (a device int64 tensor [m]; sources
        may repeat and come in any order; an entry outside 0..n-1 is "no job" and gets the word RO_NONE = 0) with its OWN tick-1
        moves `moves[j]` (a device int32 tensor [m, 4]), all by one kernel on the handle's stream; the batch is left exactly as it is
        (pom_batch_rollout_jobs, include/pom_batch.h).  Returns the result words, int32 [samples, m]: word [r, j] is what
        rollout(..., simple=, first=) writes at [r, src[j]] given moves whose row src[j] is moves[j] — every draw is keyed by the
        source env, so jobs of one source play under common random numbers and differ only through their first moves.
        `simple`, `first`, `fresh_agents`, `out`: as rollout() (the playouts are always pom_batch_rollout_policy's; with none of
        the three given: random playouts, all four tick-1 moves from `moves` if it is given)."""
        horizon, samples, dist, simple_mask, first_mask, flags = _rollout_args(horizon, samples, dist, moves, simple, first, fresh_agents)
        m = int(self._device_tensor(src, "src", "int64", (None,)).shape[0])
        out = self._out_tensor(out, (samples, m), "int32")
        self._moves(moves, shape=(m, 4))
        with self._ordered():
            spec = _spec(_RolloutJobsSpec, horizon, samples, dist, _u64(seed), m, *_job_ptrs(m, src, moves, out), simple_mask,
                         first_mask if m else 0, flags, 0)
            self._call("pom_batch_rollout_jobs", C.byref(spec))
        return out

    # ---- expand: listed games copied into slots and ticked once (pom_batch_expand) ------------------------
    def expand(self, src, moves, first: int = 0, *, out=None, codes=None, planes=None, per_agent: Optional[bool] = None,
               attrs: bool = True):
        """Create the nodes of a search in one launch: env `first + j` becomes the successor of env `src[j]` under `moves[j]` — the
        copy of copy_envs() and one tick as the handle's mode says, no restart ever played (pom_batch_expand, include/pom_batch.h).
        `src`: int64 [count], `moves`: int32 [count, 4], a row per JOB (dead agents' entries included); torch tensors on the handle's
        device, or numpy arrays, which are copied there.  An entry < 0, >= n, or inside [first, first + count) without being its own
        slot is "no job": its env is left alone and its word is RO_NONE = 0.  src[j] = first + j is a masked step of env first + j.
        Returns the result words, int32 [count] on the handle's device holding the header's uint32 words of the children as they now
        stand (decode_rollout names the fields; length 1 = ticked, 0 = the unticked copy of a finished game).  `out`: such a tensor of
        an earlier call.  `codes` (uint8 [n, 5, 11, 11]) or `planes` ([n, 16, 11, 11] or, with per_agent, [n, 4, 16, 11, 11] of uint8 /
        float16 / float32): tensors sized for the WHOLE batch into which the same launch writes the observation of the tiles of 16 envs
        the range touches; the call then returns (words, agent_attrs, env_attrs), the latter two int32 [n, 4, 8] and [n, 4] written
        for the same envs (None, None with attrs=False)."""
        def device_tensor(a, what, dtype, shape):  # numpy arrays are copied to the device, anything else is _device_tensor's
            if isinstance(a, np.ndarray):
                if not np.issubdtype(a.dtype, np.integer):
                    raise ValueError(f"{what} must be an integer array")
                torch, dev = self._torch_device()
                a = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)
            return self._device_tensor(a, what, dtype, shape)

        src = device_tensor(src, "src", "int64", (None,))
        m = int(src.shape[0])
        moves = device_tensor(moves, "moves", "int32", (m, 4))
        first, _ = self._in_batch(first, m)
        out = self._out_tensor(out, (m,), "int32")
        obs, code, per_agent, _view, width, _shape, _dtype = self._observation(codes, planes, per_agent)
        a_attrs, e_attrs = self._new_attrs(width) if obs is not None and attrs else (None, None)
        with self._ordered():
            spec = _spec(_ExpandSpec, 0, first, m, *_job_ptrs(m, src, moves, out), _ptr(obs), code, int(per_agent), _ptr(a_attrs),
                         _ptr(e_attrs), 0)
            self._call("pom_batch_expand", C.byref(spec))
        return out if obs is None else (out, a_attrs, e_attrs)

    def move_table(self, agent: int, horizon: int, samples: int, seed: int, dist: int = DIST_RANDOM, others=None, *, simple=None,
                   fresh_agents: bool = False):
        """`agent`'s six-move table in ONE rollout_jobs call of 6 n jobs: returns int32 [6, samples, n], [c, r, e] = the word of sample
        r of env e with `agent`'s tick-1 move fixed to c (0..5) — what six rollout(..., moves=, first=[agent]) calls give, stacked.
        The six playouts of an env and a sample share every draw (common random numbers): they differ through the move alone.
        `others`: a device int32 tensor [n, 4] — the other three agents' tick-1 moves are fixed to its entries too (`agent`'s own
        column is ignored); None: only `agent`'s move is fixed.  `simple`, `fresh_agents`, `dist`: as rollout()."""
        agent, n = _bounded(agent, "agent", 0, 3), self.n
        if others is not None:
            self._device_tensor(others, "others", "int32", (n, 4))
        torch, dev = self._torch_device()
        moves = torch.zeros((6, n, 4), dtype=torch.int32, device=dev) if others is None else others.unsqueeze(0).repeat(6, 1, 1)
        moves[:, :, agent] = torch.arange(6, dtype=torch.int32, device=dev).unsqueeze(1)
        src = torch.arange(n, dtype=torch.int64, device=dev).repeat(6)  # job c * n + e plays env e
        res = self.rollout_jobs(src, horizon, samples, seed, dist, moves.view(6 * n, 4), simple=0 if simple is None else simple,
                                first=0xF if others is not None else [agent], fresh_agents=fresh_agents)
        return res.view(int(samples), 6, n).permute(1, 0, 2).contiguous()

    def moves_tensor(self):
        """The handle's device move buffer as a torch int32 tensor [n, 4] (zero-copy): what policy_simple() fills and
        step_policy() consumes; overwrite entries on the handle's stream to mix in another policy."""
        torch, dev = self._torch_device()
        ptr = C.POINTER(C.c_int32)()
        self._call("pom_batch_moves_device", C.byref(ptr))
        addr = C.cast(ptr, C.c_void_p).value

        class _Raw:  # the CUDA array interface is how torch adopts foreign device memory
            __cuda_array_interface__ = {"shape": (self.n, 4), "typestr": "<i4", "data": (addr, False), "version": 2}

        t = torch.as_tensor(_Raw(), device=dev)
        # the memory belongs to the handle: the view keeps its BatchEnvironment alive (no __del__ while a view exists), and an
        # explicit close() with views outstanding is refused
        t._pom_owner = self
        self._views.append(weakref.ref(t))
        return t

    def stream_handle(self) -> int:
        """the hipStream_t (as an integer) this handle's work is ordered on"""
        s = C.c_void_p()
        self._call("pom_batch_stream", C.byref(s))
        return s.value or 0

    # ---- counters / plumbing ------------------------------------------------------------------------
    def counters(self) -> np.ndarray:
        out = np.zeros(4, dtype=np.int64)
        self._call("pom_batch_counters", out.ctypes.data)
        self._tapes.clear()
        return out

    def counters_into(self, dev_ptr: int) -> None:
        self._call("pom_batch_counters_device", dev_ptr)

    def reset_counters(self) -> None:
        self._call("pom_batch_reset_counters")

    def sync(self) -> None:
        self._call("pom_batch_sync")
        self._tapes.clear()

    def flush(self) -> None:
        """Make the handle's stream wait for all steps issued so far (host does not block)."""
        self._call("pom_batch_flush")

    def fork(self) -> None:
        """Order the internal sub-streams behind the handle's stream now (the next step then needs no cross-stream event first)."""
        if hasattr(self._lib, "pom_batch_fork"):  # (older experimental builds loaded through POM_LIB lack it)
            self._call("pom_batch_fork")

    def set_streams(self, streams: int) -> None:
        self._call("pom_batch_set_streams", streams)

    def profile(self, enable: bool) -> None:
        self._call("pom_batch_profile", int(enable))

    def _read(self, name: str, *types):
        """the values the library's `name` writes through one pointer per ctypes type of `types`"""
        outs = [t() for t in types]
        self._call(name, *map(C.byref, outs))
        return tuple(o.value for o in outs)

    def profile_read(self):
        return self._read("pom_batch_profile_read", C.c_double, C.c_int64)

    def launch_shape(self):
        """(envs per wavefront, lanes per env, launches per step)"""
        return self._read("pom_batch_launch_shape", C.c_int32, C.c_int32, C.c_int32)

    def issue_info(self):
        """(name of the issue mode in force for several-tick calls, streams their launches go to)"""
        mode, streams = self._read("pom_batch_issue_info", C.c_int32, C.c_int32)
        return {ISSUE_DIRECT: "direct", ISSUE_THREADS: "threads", ISSUE_GRAPH: "graph", ISSUE_CHAIN: "chain"}.get(mode, "?"), streams

    def device_view(self):
        return self._read("pom_batch_device_view", C.c_void_p, C.c_int64, C.c_int32)


def bench_policy(codes, moves, first: int, count: int, tick: int, stream=None) -> None:
    """pom_bench_policy: the stand-in policy of the closed-loop measurements and tests — Move[4] of the envs [first, first + count) into
    `moves` (int32[n, 4] device tensor), from the POM_OBS_CODES observation `codes` (or None: from (env, agent, tick) alone), one launch on
    `stream`."""
    lib = load_library()
    st = getattr(stream, "cuda_stream", stream)
    _check(lib, lib.pom_bench_policy(codes.data_ptr() if codes is not None else None, moves.data_ptr(), int(first), int(count), int(tick) & 0xFFFFFFFF, st))
