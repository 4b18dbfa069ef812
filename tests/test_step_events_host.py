"""pom_batch_step_events without a GPU: the hand-made cases of tests/step_events_cases.py through the checker of
tests/step_events_oracle.py — on the CPU checker's transitions and, where it was built, on the compiled reference's — give the numbers
written down there; the model plays SimpleAgent games in every reset mode and its own record holds every bit of the header's table; the
deliberately wrong variants of the model are each caught by those games; and the structure's mirror, the wrapper's argument checks and
decode_step_events() are what the header states."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pomcpp_amd
from pomcpp_amd import _abi
from pomcpp_amd.batch import BatchEnvironment, _MixedStepSpec, _StepEventsSpec
from tests import step_events_cases as SC
from tests import step_events_games as SG
from tests import step_events_oracle as EO
from tests import wrapper_standin as W
from tests.oracle_lib import Oracle
from tests.test_wrapper_args_host import _bad
from tests.wrapper_standin import Duck, N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32, U8, U32 = W.I32, W.U8, "torch.uint32"


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


# ---- the hand-made cases ---------------------------------------------------------------------------------------------------------
def _play_case(case, bboard_step, oracle):
    """[(events, outcome, wood)] of the case's ticks: every transition played by `bboard_step` (bboard::Step in place), the bookkeeping
    of Environment::Step (environment.cpp:148-168, :71) done here, the words by the checker"""
    name, mode, build, ticks = case
    s, out = build(oracle), []
    done, winner, draw, timeout = 0, -1, 0, 0
    for moves, *_ in ticks:
        if mode == "env" and done:
            out.append((EO.idle_words(s[0]), EO.outcome_word(s[0], EO.status_of(done, winner, draw, timeout)), 0))
            continue
        s0 = s.copy()
        ub = bboard_step(s, moves)
        if mode == "env":
            s["timeStep"] += 1
            alive = [a for a in range(4) if not s["agents"]["dead"][0, a]]
            winner, draw = (alive[0] if len(alive) == 1 else -1), int(not alive)
            timeout = int(s["timeStep"][0] >= SC.CAP)
            done = int(len(alive) <= 1 or timeout)
        st = EO.status_of(done, winner, draw, timeout, ub, end=bool(done))
        out.append((EO.event_words(s0[0], moves, s[0], st), EO.outcome_word(s[0], st), EO.wood_burnt(s0[0], s[0])))
    return out


def _expected(case):
    return [(list(ev), outcome, wood) for _moves, ev, outcome, wood in case[3]]


def _show(got):
    return [([hex(w) for w in ev], hex(o), wd) for ev, o, wd in got]


@pytest.mark.parametrize("case", SC.CASES, ids=SC.NAMES)
def test_hand_made_cases_through_the_checker(case, oracle):
    got = _play_case(case, lambda s, m: oracle.step(s, m), oracle)
    assert got == _expected(case), (_show(got), _show(_expected(case)))


def test_hand_made_cases_through_the_compiled_reference(oracle):
    """the same with bboard::Step of the unmodified reference where the build left it; elsewhere there is nothing to run"""
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libpomref.so")):
        return
    from tests.case_api import RefAPI
    ref = RefAPI()

    def ref_step(s, m):
        mv = np.asarray(m, dtype=np.int32)
        ref.lib.ref_step(s.ctypes.data, mv.ctypes.data)
        return 0
    for case in SC.CASES:
        got = _play_case(case, ref_step, oracle)
        assert got == _expected(case), (case[0], _show(got), _show(_expected(case)))


def test_the_cases_cover_every_clause_they_promise():
    seen = {}
    for _name, _mode, _build, ticks in SC.CASES:
        for _moves, ev, _outcome, wood in ticks:
            for w in ev:
                for k, v in EO.decode(w).items():
                    seen.setdefault(k, set()).add(v)
            seen.setdefault("wood", set()).add(wood)
    for k in ("played", "alive", "died", "moved", "laid", "gain_bomb", "gain_range", "gain_kick", "end", "won", "draw", "timeout"):
        assert seen[k] == {False, True}, k
    assert seen["exploded"] >= {0, 1} and seen["wood"] == {0, 2} and seen["move"] >= {0, 1, 2, 3, 4, 5}
    assert len(SC.group("env")) + len(SC.group("raw")) == len(SC.CASES) and len(SC.group("raw")) >= 2


# ---- the model's games -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("game", SG.GAMES, ids=SG.GAME_IDS)
def test_model_games_run_and_keep_the_handle_what_tick_mixed_leaves(game, oracle):
    """an EventsModel's handle is a MixedModel's, tick for tick: the bookkeeping of the events touches nothing"""
    from tests.mixed_model import MixedModel
    rec = SG.play(oracle, game)
    plain = SG.play(oracle, game, cls=MixedModel, ticks=SG.TICKS)
    assert not rec["model"].differences(plain["model"])
    assert len(rec["ticks"]) == SG.TICKS and rec["ticks"][0]["events"].shape == (SG.N, 4)


def test_every_bit_of_the_table_is_set_in_the_models_own_record(oracle):
    seen, exploded, moves, wood, outcome_bits = {k: 0 for k in EO.BITS}, set(), set(), set(), 0
    for game in SG.GAMES:
        for t in SG.play(oracle, game)["ticks"]:
            first, count = t["range"]
            ev = t["events"][first:first + count]
            for k, b in EO.BITS.items():
                seen[k] += int(((ev & b) != 0).sum())
            exploded |= set(np.unique(ev >> EO.EXPLODED_SHIFT & 0xF).tolist())
            moves |= set(np.unique(ev[(ev & EO.PLAYED) != 0] & EO.MOVE).tolist())
            wood |= set(np.unique(t["wood"][first:first + count]).tolist())
            outcome_bits |= int(np.bitwise_or.reduce(t["outcome"][first:first + count]))
    assert all(seen.values()), {k: v for k, v in seen.items() if not v}
    assert exploded >= {0, 1, 2} and moves >= {0, 1, 2, 3, 4, 5} and wood >= {0, 1, 2}
    assert outcome_bits & 0x7FF == 0x7FF, hex(outcome_bits)   # every alive bit, DONE, DRAW, TIMEOUT, UB and all three winner bits


class _AfterTheRestart(EO.EventsModel):
    """S1 read behind the restart at the end: the next game's start state"""

    def _s1_of(self, e, s1):
        return self.states[e]


class _LaidWithoutTheAmmoTest(EO.EventsModel):
    _laid = staticmethod(lambda a0, move: (not a0["dead"]) and move == EO.BOMB)


class _CallersMoveForTheMask(EO.EventsModel):
    def _event_moves(self, e, handed, callers, mask):
        return handed if callers is None else callers


@pytest.mark.parametrize("wrong", (_AfterTheRestart, _LaidWithoutTheAmmoTest, _CallersMoveForTheMask), ids=lambda c: c.__name__)
def test_wrong_variants_of_the_model_are_caught(wrong, oracle):
    caught = 0
    for game in SG.GAMES:
        right, other = SG.play(oracle, game), SG.play(oracle, game, cls=wrong)
        assert not right["model"].differences(other["model"])   # the handle itself is the same: only the record can tell
        caught += sum(any(a[k].tobytes() != b[k].tobytes() for k in ("events", "outcome", "wood")) for a, b in zip(right["ticks"], other["ticks"]))
    assert caught > 0


# ---- the structure, the wrapper's checks, the decoder ------------------------------------------------------------------------------
def test_the_structure_is_the_headers():
    text = open(os.path.join(ROOT, "include", "pom_batch.h")).read()
    assert C.sizeof(_StepEventsSpec) == 40 == int(re.search(r"POM_STEP_EVENTS_SPEC_SIZE = (\d+)", text).group(1))
    assert [(n, getattr(_StepEventsSpec, n).offset) for n, _ in _StepEventsSpec._fields_] == [
        ("struct_size", 0), ("flags", 4), ("events_dev", 8), ("outcome_dev", 16), ("wood_dev", 24), ("reserved_", 32)]
    assert _abi.STRUCTURES["PomStepEventsSpec"] is _StepEventsSpec
    assert "int pom_batch_step_events(PomBatch* h, const PomMixedStepSpec* step, const PomStepEventsSpec* ev);" in text
    for name, value in re.findall(r"POM_(EV_[A-Z_]+) = ([^,\n]+)", text):
        assert getattr(pomcpp_amd, name) == getattr(_abi, name) == eval(value.split("/*")[0]), name   # noqa: S307 (the header's own numbers)
    assert (pomcpp_amd.EV_END, pomcpp_amd.EV_UB, pomcpp_amd.EV_EXPLODED) == (EO.END, EO.UB, 0xF << EO.EXPLODED_SHIFT)


def _handle():
    return W.handle(BatchEnvironment)


def _specs_of(env):
    (entry, args), = env._lib.calls
    env._lib.calls.clear()
    assert entry == "pom_batch_step_events" and len(args) == 3
    step, ev = args[1]._obj, args[2]._obj
    assert isinstance(step, _MixedStepSpec) and step.struct_size == 104 and isinstance(ev, _StepEventsSpec) and ev.struct_size == 40
    assert (step.flags, step.reserved_, ev.flags, ev.reserved_) == (0, 0, 0, 0)
    return step, ev


def _rows(env):
    mv, ev = (lambda: Duck((N, 4), I32)), (lambda: Duck((N, 4), U32))  # noqa: E731
    return [
        ("events", I32, (N, 4), lambda t: env.step_events(0, 16, mv(), 0b1110, 1, 2, t)),
        ("outcome", I32, (N,), lambda t: env.step_events(0, 16, mv(), 0b1110, 1, 2, ev(), t)),
        ("wood", U8, (N,), lambda t: env.step_events(0, 16, mv(), 0b1110, 1, 2, ev(), None, t)),
        ("moves", I32, (N, 4), lambda t: env.step_events(0, 16, t, 0b1110, 1, 2, ev())),
        ("codes", U8, (N, 4, 5, 11, 11), lambda t: env.step_events(0, 16, mv(), 0b1110, 1, 2, ev(), codes=t, view_radius=4)),
    ]


def test_refused_rows_reach_no_library_function():
    env = _handle()
    wrong, n = [], 0
    for name, dtype, shape, fn in _rows(env):
        for what, t in _bad(dtype, shape):
            n += 1
            try:
                fn(t)
                wrong.append(f"{name}, {what}: accepted")
            except ValueError as e:
                if name not in str(e):
                    wrong.append(f"{name}, {what}: the text does not name {name!r}: {e}")
            if env._lib.calls:
                wrong.append(f"{name}, {what}: reached {env._lib.calls[0][0]}")
                env._lib.calls.clear()
    assert n >= 30 and not wrong, f"{len(wrong)} of {n} rows:\n" + "\n".join(wrong)
    with pytest.raises(ValueError, match="events"):
        env.step_events(0, 16, Duck((N, 4), I32), 0b1110, 1, 2, None)
    for kw in (dict(simple=16), dict(tick=-1), dict(first=8, count=N)):
        args = dict(first=0, count=16, moves=Duck((N, 4), I32), simple=0b1110, seed=1, tick=2, events=Duck((N, 4), U32))
        with pytest.raises(ValueError):
            env.step_events(**dict(args, **kw))
    assert not env._lib.calls


def test_right_tensors_reach_the_one_entry_point_with_the_fields_as_given():
    env = _handle()
    mv, ev, oc, wd = Duck((N, 4), I32), Duck((N, 4), U32), Duck((N,), I32), Duck((N,), U8)
    env.step_events(16, 4, mv, [1, 3], (1 << 64) + 5, 0xFFFFFFFF, ev, oc, wd, 0x77)
    step, spec = _specs_of(env)
    assert (step.simple_mask, step.first, step.count, step.moves_dev, step.seed, step.tick, step.stream) == (0b1010, 16, 4, mv.address, 5, 0xFFFFFFFF, 0x77)
    assert (spec.events_dev, spec.outcome_dev, spec.wood_dev) == (ev.address, oc.address, wd.address) and not step.view and not step.planes_dev
    views, va, ea = Duck((N, 4, 5, 11, 11), U8), Duck((N, 4, 12), I32), Duck((N, 4), I32)
    env.step_events(0, N, None, 0xF, 7, 0, Duck((N, 4), I32), codes=views, view_radius=4, viewer_attrs=va, env_attrs=ea)   # int32 events too
    step, spec = _specs_of(env)
    v = step.view.contents
    assert (step.simple_mask, step.moves_dev, spec.outcome_dev, spec.wood_dev) == (15, None, None, None)
    assert (v.view_radius, v.dtype, v.planes_dev, v.viewer_attrs_dev, v.env_attrs_dev) == (4, 3, views.address, va.address, ea.address)
    env.step_events(0, 0, 0x1000, 0, 7, 3, 0x2000, 0x3000, 0x4000)   # raw addresses pass unchecked
    step, spec = _specs_of(env)
    assert (step.moves_dev, spec.events_dev, spec.outcome_dev, spec.wood_dev) == (0x1000, 0x2000, 0x3000, 0x4000)


def test_step_mixed_and_step_events_build_the_same_step_spec():
    env = _handle()
    mv, planes, a, e = Duck((N, 4), I32), Duck((N, 4, 16, 11, 11), W.F16), Duck((N, 4, 8), I32), Duck((N, 4), I32)
    env.step_mixed(16, 4, mv, 0b0110, 9, 11, 0x55, planes=planes, per_agent=True, agent_attrs=a, env_attrs=e)
    (_, args), = env._lib.calls
    env._lib.calls.clear()
    env.step_events(16, 4, mv, 0b0110, 9, 11, Duck((N, 4), U32), stream=0x55, planes=planes, per_agent=True, agent_attrs=a, env_attrs=e)
    step, _ = _specs_of(env)
    assert bytes(args[1]._obj) == bytes(step)


def test_decode_step_events_names_the_fields():
    words = np.array([[0x9D, 0x51028], [0x10, 0x190F5C]], dtype=np.uint32)
    for w in (words, words.view(np.int32)):
        d = pomcpp_amd.decode_step_events(w)
        assert d["move"].tolist() == [[5, 0], [0, 4]] and d["exploded"].tolist() == [[0, 1], [0, 0]] and d["move"].dtype == np.int32
        assert d["laid"].tolist() == [[True, False], [False, False]] and d["died"].tolist() == [[False, True], [False, False]]
        assert d["end"].tolist() == [[False, True], [False, True]] and d["draw"].tolist() == [[False, True], [False, False]]
        assert d["timeout"].tolist() == [[False, False], [False, True]] and d["ub"].tolist() == [[False, False], [False, True]]
        assert d["played"].tolist() == [[True, True], [False, True]] and d["alive"].tolist() == [[True, False], [True, True]]
        assert d["restarted"].tolist() == [[False, False], [False, True]] and d["gain_kick"].tolist() == [[False, False], [False, True]]
        for k in ("moved", "gain_bomb", "gain_range", "won"):
            assert d[k].tolist() == [[False, False], [False, k != "won"]], k
        for k, b in EO.BITS.items():
            assert np.array_equal(d[k], (words & b) != 0), k
