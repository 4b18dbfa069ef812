"""The queue loops every tick runs — flames_dec, flame_pops, the scan of the bombs under agents and the bomb pass
(pomcpp_amd/csrc/pom_step_body.h) — on the hand-made corpus of tests/queue_first_trip_cases.py, without a GPU.

With a quad per env the first trip of each of these loops is played straight-line (lane `sub` takes queue offset `sub`) and only
offsets 4 and up go through the loop.  Every entry is played through the four-lane host model of the device tick (the shipped shape,
with its rendezvous checks: tests/emul/pom_emul_quad.cpp) and through the one-lane build, every tick against the oracle: all 1004
bytes and the tick's flags, no entry and no tick left out.  The record holds a flame timer at -128 where the reference's falls
further (include/pom_state.h): the expected state has it there (queue_first_trip_cases.traces).  The corpus is recounted from the
oracle's own run, so that an entry that no longer reaches what it is for is noticed.  The same corpus runs through the kernels in
tests/test_gpu_queue_first_trip.py."""
import ctypes as C

import numpy as np
import pytest

from pomcpp_amd.state import STATE_DTYPE, Item
from tests import queue_first_trip_cases as QC
from tests.edge_states import FATAL, UB_FLAME_QUEUE_RANGE
from tests.test_emul import emul_bins  # noqa: F401  (the host builds of the device body)

T = QC.TICKS


class Stage:
    def __init__(self, oracle):
        self.entries = QC.corpus(oracle)
        self.names = [e.name for e in self.entries]
        self.ix = {n: i for i, n in enumerate(self.names)}
        self.states, self.ubs = QC.traces(oracle, self.entries)
        self.sticky = np.bitwise_or.accumulate(self.ubs, axis=1)

    def field(self, name, field):
        """a State field of an entry at the start and after every tick: [T + 1, ...]"""
        i = self.ix[name]
        after = self.states[i].view(STATE_DTYPE)[:, 0][field]
        return np.concatenate([self.entries[i].start[field], after])


@pytest.fixture(scope="module")
def stage(oracle):
    return Stage(oracle)


def _run(lib, e, quad):
    run = lib.pom_emul_run
    run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    run.restype = C.c_int
    got, ubs = np.zeros((T, 1004), dtype=np.uint8), np.zeros(T, dtype=np.uint32)
    mv = np.ascontiguousarray(e.moves, dtype=np.int32)
    assert run(e.start.ctypes.data, mv.ctypes.data, T, quad, got.ctypes.data, ubs.ctypes.data) == 0, f"{e.name}: upload refuses the start state"
    return got, ubs


@pytest.mark.parametrize("quad", [1, 0], ids=["quad", "one_lane"])
def test_device_tick_body_matches_oracle_on_every_entry(emul_bins, stage, quad):  # noqa: F811
    """every tick of every entry, the record packed once and kept between the ticks as a device buffer keeps it"""
    for i, e in enumerate(stage.entries):
        got, ubs = _run(emul_bins, e, quad)
        assert not (ubs & 0x40000000).any(), f"{e.name}: the quad model's checks failed (ticks {np.nonzero(ubs & 0x40000000)[0].tolist()})"
        assert np.array_equal(ubs, stage.ubs[i]), f"{e.name}: ubflags {ubs.tolist()}, oracle {stage.ubs[i].tolist()}"
        bad = np.nonzero((got != stage.states[i]).any(axis=1))[0]
        assert bad.size == 0, f"{e.name} tick {bad[0]}: bytes {np.nonzero(got[bad[0]] != stage.states[i, bad[0]])[0][:12].tolist()} differ"


def test_no_entry_raises_a_fatal_flag_and_the_held_timers_are_flagged(stage):
    for e, ubs in zip(stage.entries, stage.ubs):
        seen = int(np.bitwise_or.reduce(ubs))
        assert not seen & FATAL, e.name
        assert seen & e.expect_ub == e.expect_ub, e.name
        assert bool(seen & UB_FLAME_QUEUE_RANGE) == e.name.startswith("fl_minus128"), e.name
    # -127 reaches -128 with the reference's value still in the record: the flag comes one tick later than with -128 at the start
    assert stage.ubs[stage.ix["fl_minus128_reaches_offset0"], 0] == 0 and stage.ubs[stage.ix["fl_minus128_reaches_offset0"], 1] == UB_FLAME_QUEUE_RANGE
    assert stage.ubs[stage.ix["fl_minus128_held_offset5"], 0] == UB_FLAME_QUEUE_RANGE


def test_the_flame_entries_reach_what_they_are_for(stage):
    counts = {int(e.start["flames_count"][0]) for e in stage.entries if e.name.startswith("fl_")}
    assert {0, 1, 3, 4, 5, 8, 20} <= counts and max(counts) > 20
    heads = {int(e.start["flames_index"][0]) for e in stage.entries if e.name.startswith("fl_") and int(e.start["flames_count"][0]) > 0}
    assert {17, 18, 19} <= heads
    # two flames run out in one tick, from a queue that fits the first trip and from one that does not
    for name in ("fl_count4_head17", "fl_count8_head17", "fl_count20_head19"):
        c = stage.field(name, "flames_count")
        assert (np.diff(c) == -2).any(), (name, c.tolist())
    # nothing pops while the head is young
    c = stage.field("fl_count8_head19_young", "flames_count")
    assert c[:4].tolist() == [8, 8, 8, 8] and c[4] == 0
    # above 20 the queue stays (the head's slot is visited twice: edge_states) or pops by more than the first trip covers
    assert stage.field("fl_count21_head17_time3", "flames_count")[-1] > 20
    # arms: the corpus's flames leave no flame cell behind once they are gone, and the flagged ones leave their power-ups
    for name in ("fl_arms_head0", "fl_arms_head17", "fl_flagged_first_cell", "fl_flagged_second_cell"):
        i = stage.ix[name]
        assert (stage.entries[i].start["board"] >> 16 == 4).sum() >= 9, name
        last = stage.states[i, T - 1].view(STATE_DTYPE)[0]
        assert int(last["flames_count"]) == 0 and not (last["board"] >> 16 == 4).any(), name
    for name, dist in (("fl_flagged_first_cell", 1), ("fl_flagged_second_cell", 2)):
        i = stage.ix[name]
        b0 = stage.entries[i].start["board"][0]
        flagged = [(x, y) for y in range(11) for x in range(11) if (b0[y, x] >> 16) == 4 and (b0[y, x] & 7)]
        assert len(flagged) >= 6, (name, flagged)
        assert all(min(abs(x - ox) + abs(y - oy) for ox, oy in ((5, 5), (1, 1), (9, 9))) == dist for x, y in flagged), (name, flagged)
        last = stage.states[i, T - 1].view(STATE_DTYPE)[0]["board"]
        assert {int(last[y, x]) for x, y in flagged} == {Item.EXTRABOMB, Item.INCRRANGE, Item.KICK}, name
    strengths = {int(f["strength"]) for f in stage.entries[stage.ix["fl_arms_head0"]].start["flames_queue"][0][:8]}
    assert strengths == {0, 1, 2, 3}


def test_the_bomb_entries_reach_what_they_are_for(stage):
    counts = {int(e.start["bombs_count"][0]) for e in stage.entries if e.name.startswith("bo_count")}
    assert {0, 1, 4, 5, 8, 20} <= counts
    heads = {int(e.start["bombs_index"][0]) for e in stage.entries if e.name.startswith("bo_")}
    assert {17, 18, 19} <= heads
    # `late`: the bomb with timer 0 behind the head goes off only when it has become the head or a blast reaches it; its word is
    # decremented after loop B, which shows as a timer nibble of 15 after the first tick
    for at in (1, 5):
        q = stage.field(f"bo_late_offset{at}", "bombs_queue")
        assert (int(q[0, (18 + at) % 20]) >> 16) & 0xF == 0 and (int(q[1, (18 + at) % 20]) >> 16) & 0xF == 15, at
    # an agent that walked onto a resting bomb is back where he stood (bounced), tick after tick
    for at in (0, 3, 4, 7):
        a = stage.field(f"bo_walked_onto_offset{at}", "agents")
        assert [int(v) for v in a[:3, 0]["x"]] == [4, 4, 4], at
    # ... and one who walks off the bomb he stood on leaves a BOMB item behind
    for at in (0, 3, 4, 7):
        b = stage.field(f"bo_left_behind_offset{at}", "board")
        assert int(b[0, 5, 5]) == Item.AGENT1 and int(b[1, 5, 5]) == Item.BOMB and int(b[1, 5, 6]) == Item.AGENT1, at
    # moving bombs move; the kicked one too
    for name, at, index in (("bo_moving_offset0", 0, 18), ("bo_moving_offset4", 4, 18), ("bo_kicked_offset5", 5, 19)):
        q = stage.field(name, "bombs_queue")
        assert (int(q[0, (index + at) % 20]) & 0xFF) != (int(q[1, (index + at) % 20]) & 0xFF), name
    # a plant of the first tick lands in the slot its name says, with a direction inherited from the stale word
    for have, index in ((4, 17), (1, 19), (5, 18), (3, 19)):
        name = f"bo_planted_into_offset{have}_head{index}"
        c = stage.field(name, "bombs_count")
        assert c[0] == have and c[1] == have + 1, (name, c.tolist())
        b = int(stage.field(name, "bombs_queue")[1, (index + have) % 20])
        assert (b >> 8) & 0xF == 0, name  # agent 0's
    # the queues that go off from the head lose two bombs in a tick
    for name in ("bo_count5_head19_ripe", "bo_count8_head17_ripe"):
        c = stage.field(name, "bombs_count")
        assert (np.diff(c) <= -2).any(), (name, c.tolist())
