"""The ctypes mirror of include/pom_batch.h, and nothing else: its constants, its spec structures with their builders, the
prototype of every function it declares (PROTOTYPES) and the loading of libpom_batch.so.  Whatever is written here is written a
second time in the header; tests/test_abi_mirror.py compares the two, field by field and argument by argument, without the library.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
MODE_RAW, MODE_ENV = 0, 1
RESET_OFF, RESET_AT_START, RESET_AT_END = 0, 1, 2  # PomBatchOptions.auto_reset (True = RESET_AT_START)
DIST_HARMLESS, DIST_RANDOM, DIST_STRESS = 0, 1, 2
CNT_STEPS, CNT_EPISODES, CNT_RESETS, CNT_UB_TICKS = 0, 1, 2, 3
ISSUE_AUTO, ISSUE_DIRECT, ISSUE_THREADS, ISSUE_GRAPH, ISSUE_CHAIN = 0, 1, 2, 3, 4  # PomBatchOptions.issue_mode
COPY_FROM_SNAPSHOT, COPY_SET_SNAPSHOT = 1, 2  # pom_batch_copy_envs flags
UB_LOST_AGENT, UB_NULL_BOMB, UB_QUEUE_OVERFLOW, UB_REVERT_LOOP, UB_BAD_INDEX, UB_FLAME_QUEUE_RANGE = 1, 2, 4, 8, 16, 32
ROLLOUT_FRESH_AGENTS = 1  # POM_ROLLOUT_FRESH_AGENTS
REACH_MAX_DIST = 120  # POM_REACH_MAX_DIST
MEMORY_PLANES, MEMORY_AGE_NEVER, MEMORY_AGE_MAX = 6, 255, 254  # POM_MEMORY_*: a remembered view's planes, the age plane's two ends
IMAGINE_SAMPLE, IMAGINE_PASSAGE = 0, 1  # POM_IMAGINE_*: how pom_batch_imagine fills a never-seen cell
# its result word: POM_IMAGINE_BUILT, _DROPPED_BOMBS, _DROPPED_FLAMES, _NO_ROOM, _UNKNOWN_SHIFT, _DRAWN_SHIFT
IMAGINE_BUILT, IMAGINE_DROPPED_BOMBS, IMAGINE_DROPPED_FLAMES, IMAGINE_NO_ROOM, IMAGINE_UNKNOWN_SHIFT, IMAGINE_DRAWN_SHIFT = 1, 2, 4, 8, 8, 16
DEAL_START, DEAL_NEXT = 0, 1  # POM_DEAL_*: what a dealt env receives (PomDealSpec.mode)
DEAL_ALL, DEAL_MASK, DEAL_RESTARTED, DEAL_DONE = 0, 1, 2, 3  # which envs of the range are dealt (PomDealSpec.which)
LAYOUT_NO_LANES = 1  # POM_LAYOUT_NO_LANES
DEAL_DEALT, DEAL_FALLBACK, DEAL_ATTEMPTS_SHIFT, DEAL_BAD_SHIFT = 1, 2, 8, 16  # pom_batch_deal's result word
VIEW_CENTRED = 1  # POM_VIEW_CENTRED (PomCompactViewSpec.flags)
RO_NONE = 0  # POM_RO_NONE: rollout_jobs' word of an entry without a job
# the result word of a rollout (the header's POM_RO_*)
RO_ALIVE, RO_DONE, RO_DRAW, RO_TIMEOUT, RO_UB, RO_WINNER_SHIFT, RO_WINNER_MASK, RO_LENGTH_SHIFT = 0xF, 0x10, 0x20, 0x40, 0x80, 8, 0x700, 16
# a step's event word (the header's POM_EV_*, PomStepEventsSpec)
(EV_MOVE, EV_PLAYED, EV_ALIVE, EV_DIED, EV_MOVED, EV_LAID, EV_GAIN_BOMB, EV_GAIN_RANGE, EV_GAIN_KICK, EV_RESTARTED, EV_EXPLODED_SHIFT,
 EV_EXPLODED, EV_END, EV_WON, EV_DRAW, EV_TIMEOUT, EV_UB) = (0x7, 1 << 3, 1 << 4, 1 << 5, 1 << 6, 1 << 7, 1 << 8, 1 << 9, 1 << 10, 1 << 11, 12,
                                                                0xF << 12, 1 << 16, 1 << 17, 1 << 18, 1 << 19, 1 << 20)


class PomError(RuntimeError):
    def __init__(self, code: int, text: str):
        super().__init__(f"pom_batch error {code}: {text}")
        self.code = code


class _Options(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("device", C.c_int32), ("stream", C.c_void_p),
        ("mode", C.c_int32), ("auto_reset", C.c_int32), ("max_steps", C.c_int32),
        ("env_offset", C.c_int64), ("envs_per_wave", C.c_int32), ("streams", C.c_int32),
        ("lanes_per_env", C.c_int32), ("fresh_boards", C.c_int32), ("board_seed", C.c_uint64),
        ("issue_mode", C.c_int32), ("reserved_", C.c_int32),
    ]


class _ViewSpec(C.Structure):
    """PomViewSpec (include/pom_batch.h): where the fogged per-agent views go"""
    _fields_ = [
        ("struct_size", C.c_int32), ("dtype", C.c_int32), ("view_radius", C.c_int32), ("reserved_", C.c_int32),
        ("planes_dev", C.c_void_p), ("viewer_attrs_dev", C.c_void_p), ("env_attrs_dev", C.c_void_p),
    ]


class _CompactViewSpec(C.Structure):
    """PomCompactViewSpec (include/pom_batch.h): a PomViewSpec whose struct_size says 56, then whose views are written and how.  It
    grows PomViewSpec and has no struct_size member of its own, so STRUCTURES — the specs that begin with one — does not list it"""
    _fields_ = [("view", _ViewSpec), ("viewer_mask", C.c_int32), ("flags", C.c_int32), ("reserved2_", C.c_int64)]


class _ForecastSpec(C.Structure):
    """PomForecastSpec (include/pom_batch.h): the forecast's horizon, first-tick moves and outputs"""
    _fields_ = [
        ("struct_size", C.c_int32), ("horizon", C.c_int32), ("reserved_", C.c_int32 * 2),
        ("moves_dev", C.c_void_p), ("flame_tick_dev", C.c_void_p), ("agent_tick_dev", C.c_void_p), ("ubflags_dev", C.c_void_p),
    ]


class _MoveSafetySpec(C.Structure):
    """PomMoveSafetySpec (include/pom_batch.h): the horizon, whose moves are judged, the others' first-tick moves and the two outputs"""
    _fields_ = [
        ("struct_size", C.c_int32), ("horizon", C.c_int32), ("agent_mask", C.c_int32), ("reserved_", C.c_int32),
        ("moves_dev", C.c_void_p), ("death_tick_dev", C.c_void_p), ("escape_tick_dev", C.c_void_p), ("reserved2_", C.c_int64),
    ]


class _ReachSpec(C.Structure):
    """PomReachSpec (include/pom_batch.h): whose reachability maps are computed, how far, and the two outputs"""
    _fields_ = [
        ("struct_size", C.c_int32), ("agent_mask", C.c_int32), ("max_dist", C.c_int32), ("reserved_", C.c_int32),
        ("dist_dev", C.c_void_p), ("move_dev", C.c_void_p), ("reserved2_", C.c_int64),
    ]


class _MemorySpec(C.Structure):
    """PomMemorySpec (include/pom_batch.h): the window, whose memory is updated, the memory and its stamps, the attribute outputs"""
    _fields_ = [
        ("struct_size", C.c_int32), ("view_radius", C.c_int32), ("agent_mask", C.c_int32), ("reserved_", C.c_int32),
        ("memory_dev", C.c_void_p), ("stamp_dev", C.c_void_p), ("viewer_attrs_dev", C.c_void_p), ("env_attrs_dev", C.c_void_p),
    ]


class _ImagineSpec(C.Structure):
    """PomImagineSpec (include/pom_batch.h): the range of slots, the job list, the view memory it builds from, the draws, the result"""
    _fields_ = [
        ("struct_size", C.c_int32), ("unknown", C.c_int32), ("first", C.c_int64), ("count", C.c_int64), ("rows", C.c_int32),
        ("reserved_", C.c_int32), ("seed", C.c_uint64), ("view_dev", C.c_void_p), ("sample_dev", C.c_void_p), ("memory_dev", C.c_void_p),
        ("viewer_attrs_dev", C.c_void_p), ("belief_attrs_dev", C.c_void_p), ("result_dev", C.c_void_p), ("stream", C.c_void_p),
    ]


class _BoardLayout(C.Structure):
    """PomBoardLayout (include/pom_batch.h): the counts of a dealt board; no spec of its own, a member of PomDealSpec"""
    _fields_ = [("num_rigid", C.c_int32), ("num_wood", C.c_int32), ("num_items", C.c_int32), ("max_inaccessible", C.c_int32), ("flags", C.c_int32)]


class _DealSpec(C.Structure):
    """PomDealSpec (include/pom_batch.h): what a dealt env receives, which envs of the range are dealt, the draws' seed, the layout, the
    game counters, the mask, the result words, the stream"""
    _fields_ = [
        ("struct_size", C.c_int32), ("mode", C.c_int32), ("which", C.c_int32), ("reserved_", C.c_int32), ("first", C.c_int64),
        ("count", C.c_int64), ("seed", C.c_uint64), ("layout", _BoardLayout), ("reserved2_", C.c_int32), ("games_dev", C.c_void_p),
        ("which_dev", C.c_void_p), ("result_dev", C.c_void_p), ("stream", C.c_void_p),
    ]


class _RolloutSpec(C.Structure):
    """PomRolloutSpec (include/pom_batch.h): the rollout's horizon, samples, move stream, first-tick moves and result"""
    _fields_ = [
        ("struct_size", C.c_int32), ("horizon", C.c_int32), ("samples", C.c_int32), ("dist", C.c_int32), ("seed", C.c_uint64),
        ("moves_dev", C.c_void_p), ("result_dev", C.c_void_p), ("reserved_", C.c_int64),
    ]


class _RolloutPolicySpec(C.Structure):
    """PomRolloutPolicySpec (include/pom_batch.h): the rollout's spec plus who plays SimpleAgent, whose first move is fixed, and flags"""
    _fields_ = [
        ("struct_size", C.c_int32), ("horizon", C.c_int32), ("samples", C.c_int32), ("dist", C.c_int32), ("seed", C.c_uint64),
        ("moves_dev", C.c_void_p), ("result_dev", C.c_void_p), ("simple_mask", C.c_int32), ("first_mask", C.c_int32),
        ("flags", C.c_int32), ("reserved_", C.c_int32),
    ]


class _RolloutJobsSpec(C.Structure):
    """PomRolloutJobsSpec (include/pom_batch.h): the policy rollout's spec for a device-side list of (source env, tick-1 moves)"""
    _fields_ = [
        ("struct_size", C.c_int32), ("horizon", C.c_int32), ("samples", C.c_int32), ("dist", C.c_int32), ("seed", C.c_uint64),
        ("jobs", C.c_int64), ("src_dev", C.c_void_p), ("moves_dev", C.c_void_p), ("result_dev", C.c_void_p),
        ("simple_mask", C.c_int32), ("first_mask", C.c_int32), ("flags", C.c_int32), ("reserved_", C.c_int32),
    ]


class _ExpandSpec(C.Structure):
    """PomExpandSpec (include/pom_batch.h): env first + j becomes the successor of env src[j] under moves[j]"""
    _fields_ = [
        ("struct_size", C.c_int32), ("flags", C.c_int32), ("first", C.c_int64), ("count", C.c_int64), ("src_dev", C.c_void_p),
        ("moves_dev", C.c_void_p), ("result_dev", C.c_void_p), ("planes_dev", C.c_void_p), ("dtype", C.c_int32), ("per_agent", C.c_int32),
        ("agent_attrs_dev", C.c_void_p), ("env_attrs_dev", C.c_void_p), ("reserved_", C.c_int64),
    ]


class _MixedStepSpec(C.Structure):
    """PomMixedStepSpec (include/pom_batch.h): one tick of a range, SimpleAgent for the agents of simple_mask, the others' moves, the
    stream, and the observation as a PomViewSpec or as the range call's plain outputs"""
    _fields_ = [
        ("struct_size", C.c_int32), ("simple_mask", C.c_int32), ("first", C.c_int64), ("count", C.c_int64), ("moves_dev", C.c_void_p),
        ("seed", C.c_uint64), ("tick", C.c_int64), ("stream", C.c_void_p), ("view", C.POINTER(_ViewSpec)), ("planes_dev", C.c_void_p),
        ("dtype", C.c_int32), ("per_agent", C.c_int32), ("agent_attrs_dev", C.c_void_p), ("env_attrs_dev", C.c_void_p),
        ("flags", C.c_int32), ("reserved_", C.c_int32),
    ]


class _StepEventsSpec(C.Structure):
    """PomStepEventsSpec (include/pom_batch.h): where pom_batch_step_events writes the agents' event words, the envs' outcome words and
    the burnt-wood counts"""
    _fields_ = [
        ("struct_size", C.c_int32), ("flags", C.c_int32), ("events_dev", C.c_void_p), ("outcome_dev", C.c_void_p), ("wood_dev", C.c_void_p),
        ("reserved_", C.c_int64),
    ]


STRUCTURES = {"PomBatchOptions": _Options, "PomViewSpec": _ViewSpec, "PomForecastSpec": _ForecastSpec,
              "PomMoveSafetySpec": _MoveSafetySpec, "PomReachSpec": _ReachSpec, "PomMemorySpec": _MemorySpec, "PomImagineSpec": _ImagineSpec, "PomDealSpec": _DealSpec, "PomRolloutSpec": _RolloutSpec,
              "PomRolloutPolicySpec": _RolloutPolicySpec, "PomRolloutJobsSpec": _RolloutJobsSpec, "PomExpandSpec": _ExpandSpec, "PomMixedStepSpec": _MixedStepSpec,
              "PomStepEventsSpec": _StepEventsSpec}  # the header's name of each


def _ptr(t):
    """what a spec's pointer field takes: None, a tensor's device address, or a raw address"""
    return None if t is None else t.data_ptr() if hasattr(t, "data_ptr") else int(t)


def _spec(cls, *fields):
    """a spec of `cls` with its struct_size filled in and the fields after it as given"""
    return cls(C.sizeof(cls), *fields)


def _view_spec(code: int, radius: int, planes, viewer_attrs=None, env_attrs=None, compact=None) -> _ViewSpec:
    """the spec of the fogged views; `compact` = (viewer_mask, flags): the PomViewSpec a PomCompactViewSpec begins with (&spec.view,
    which keeps the whole spec alive)"""
    if compact is None:
        return _spec(_ViewSpec, code, int(radius), 0, _ptr(planes), _ptr(viewer_attrs), _ptr(env_attrs))
    head = _ViewSpec(C.sizeof(_CompactViewSpec), code, int(radius), 0, _ptr(planes), _ptr(viewer_attrs), _ptr(env_attrs))
    return _CompactViewSpec(head, int(compact[0]), int(compact[1]), 0).view


def _forecast_spec(horizon: int, moves, flame_tick, agent_tick=None, ubflags=None) -> _ForecastSpec:
    return _spec(_ForecastSpec, int(horizon), (C.c_int32 * 2)(0, 0), _ptr(moves), _ptr(flame_tick), _ptr(agent_tick), _ptr(ubflags))


_P, _I32, _I64, _U64, _VP = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_void_p  # _P: the handle, _VP: any other pointer
PROTOTYPES = (  # (name, argtypes or None: no parameters, restype or None: int)
    ("pom_last_error", None, C.c_char_p), ("pom_device_count", None, C.c_int),
    ("pom_batch_create", [C.POINTER(_P), _I64, C.POINTER(_Options)], None), ("pom_batch_destroy", [_P], None),
    ("pom_batch_size", [_P], _I64),
    ("pom_batch_observe", [_P, _VP, _I32, _I32, _VP, _VP], None),
    ("pom_batch_step_device_observe", [_P, _VP, _VP, _I32, _I32, _VP, _VP], None),
    ("pom_batch_observe_view", [_P, C.POINTER(_ViewSpec)], None),
    ("pom_batch_step_device_observe_view", [_P, _VP, C.POINTER(_ViewSpec)], None),
    ("pom_batch_step_device_range_view", [_P, _I64, _I64, _VP, _VP, C.POINTER(_ViewSpec)], None),
    ("pom_batch_step_mixed", [_P, C.POINTER(_MixedStepSpec)], None),
    ("pom_batch_step_events", [_P, C.POINTER(_MixedStepSpec), C.POINTER(_StepEventsSpec)], None),
    ("pom_batch_forecast", [_P, C.POINTER(_ForecastSpec)], None),
    ("pom_batch_rollout", [_P, C.POINTER(_RolloutSpec)], None),
    ("pom_batch_rollout_policy", [_P, C.POINTER(_RolloutPolicySpec)], None),
    ("pom_batch_rollout_jobs", [_P, C.POINTER(_RolloutJobsSpec)], None),
    ("pom_batch_expand", [_P, C.POINTER(_ExpandSpec)], None),
    ("pom_batch_move_safety", [_P, C.POINTER(_MoveSafetySpec)], None),
    ("pom_batch_reach", [_P, C.POINTER(_ReachSpec)], None),
    ("pom_batch_remember_view", [_P, _I64, _I64, C.POINTER(_MemorySpec), _VP], None),
    ("pom_batch_imagine", [_P, C.POINTER(_ImagineSpec)], None),
    ("pom_batch_deal", [_P, C.POINTER(_DealSpec)], None),
    ("pom_batch_step_device_range", [_P, _I64, _I64, _VP, _VP, _VP, _I32, _I32, _VP, _VP], None),
    ("pom_bench_policy", [_VP, _VP, _I64, _I64, C.c_uint32, _VP], None),
    ("pom_batch_stream", [_P, C.POINTER(C.c_void_p)], None),
    ("pom_batch_moves_device", [_P, C.POINTER(C.POINTER(C.c_int32))], None),
    ("pom_batch_generate", [_P, _U64], None), ("pom_batch_episodes", [_P, _I64, _I64, _VP], None),
    ("pom_batch_upload", [_P, _VP, _I64, _I64], None), ("pom_batch_download", [_P, _VP, _I64, _I64], None),
    ("pom_batch_snapshot", [_P], None),
    ("pom_batch_copy_envs", [_P, _VP, _I64, _I64, _I32], None), ("pom_batch_copy_envs_device", [_P, _VP, _I64, _I64, _I32], None),
    ("pom_batch_step", [_P, _VP], None), ("pom_batch_step_device", [_P, _VP], None),
    ("pom_batch_step_device_many", [_P, _VP, _I32], None), ("pom_batch_chain_stats", [_P, _VP], None),
    ("pom_batch_step_random", [_P, _U64, _I32, _I32, _I32], None), ("pom_batch_set_tick", [_P, _I64], None),
    ("pom_batch_policy_simple", [_P, _U64, _VP], None), ("pom_batch_step_policy", [_P], None),
    ("pom_batch_step_simple", [_P, _U64, _I32], None), ("pom_batch_policy_memory", [_P, _I64, _I64, _VP], None),
    ("pom_batch_status", [_P, _I64, _I64, _VP, _VP, _VP, _VP, _VP, _VP], None),
    ("pom_batch_last_results", [_P, _I64, _I64, _VP, _VP, _VP, _VP, _VP], None),
    ("pom_batch_download_terminal", [_P, _VP, _I64, _I64], None),
    ("pom_batch_counters", [_P, _VP], None), ("pom_batch_counters_device", [_P, _VP], None),
    ("pom_batch_reset_counters", [_P], None), ("pom_batch_sync", [_P], None), ("pom_batch_flush", [_P], None),
    ("pom_batch_fork", [_P], None), ("pom_batch_set_streams", [_P, _I32], None), ("pom_batch_profile", [_P, C.c_int], None),
    ("pom_batch_profile_read", [_P, C.POINTER(C.c_double), C.POINTER(_I64)], None),
    ("pom_batch_launch_shape", [_P, C.POINTER(_I32), C.POINTER(_I32), C.POINTER(_I32)], None),
    ("pom_batch_issue_info", [_P, C.POINTER(_I32), C.POINTER(_I32)], None),
    ("pom_batch_device_view", [_P, C.POINTER(_VP), C.POINTER(_I64), C.POINTER(_I32)], None),
    ("pom_chain_litmus", [_I32, _I64, _I32, _I32, _VP], None),
    ("pom_step", [_VP, _VP], None), ("pom_env_step", [_VP, _VP, _I32, _VP, _VP, _VP, _VP], None),
)


def library_path() -> str:
    return os.environ.get("POM_LIB") or os.path.join(_HERE, "libpom_batch.so")  # POM_LIB: experimental builds only


_lib = None


def load_library() -> C.CDLL:
    """Load the HIP extension built in-tree by `__graft_entry__.build()`; fail loudly if absent."""
    global _lib
    if _lib is not None:
        return _lib
    # torch-ROCm wheels carry their own HIP runtime.  A process that is going to use both (observe(), bench.py) must load
    # torch's first so that this library binds to the same runtime; the other order leaves torch without a device.
    if "torch" not in sys.modules and not os.environ.get("POM_NO_TORCH"):
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    path = library_path()
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build the gfx950 extension first (python -c 'import __graft_entry__ as g; g.build()'). "
            "pomcpp_amd has no CPU stepper to fall back to.")
    lib = C.CDLL(path)
    lenient = bool(os.environ.get("POM_LIB"))  # an older experimental build may lack the newer calls: a missing symbol is skipped
    for name, argtypes, restype in PROTOTYPES:
        if lenient and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)  # (the project's own library: a missing symbol raises)
        if argtypes is not None:
            fn.argtypes = argtypes
        if restype is not None:
            fn.restype = restype
    _lib = lib
    return lib


def _check(lib, rc: int) -> None:
    if rc != 0:
        raise PomError(rc, lib.pom_last_error().decode(errors="replace"))
