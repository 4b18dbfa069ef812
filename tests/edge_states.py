"""A directed corpus of states at the limits of the device record (pomcpp_amd/csrc/pom_packed.h) — test infrastructure.

Random play (oracle/pom_testgen.h scenarios 0..3) keeps every narrow field of the record far from its width.  Each entry here
starts at or next to a limit and carries a Move[4] script that pushes toward it:
  - the flame queue with more than 20 entries (the head's slot is visited once per 20 entries, so the head can step over 0 and
    the queue gets stuck), timeLeft past -128 and count past 255 (POM_UB_FLAME_QUEUE_RANGE), explosions while stuck;
  - bombCount, maxBombCount, bombStrength and aliveAgents at their upload bounds and one inside them, with plants, explosions,
    pick-ups and deaths that move them;
  - values at their limits that must keep agreeing: bomb strengths that spill into the time nibble, flame strength 255 at the
    board's edges, flagged flame cells 10 cells from their origin, wood flags under flames, a full bomb queue, and entries that
    raise LOST_AGENT, NULL_BOMB and QUEUE_OVERFLOW.  (REVERT_LOOP and BAD_INDEX have none yet: no uploadable state found so far
    reaches them.)

corpus(oracle) is deterministic: the same entries, states and scripts every time.  tests/golden/gen_edge_cases.py runs it
through the compiled reference; tests/test_record_edges.py through the oracle, the host builds of the device tick and the GPU.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import pomcpp_amd.state as S
from pomcpp_amd.state import Item, Move

I, U, D, L, R, B = Move.IDLE, Move.UP, Move.DOWN, Move.LEFT, Move.RIGHT, Move.BOMB

# POM_UB_* (include/pom_state.h)
UB_LOST_AGENT, UB_NULL_BOMB, UB_QUEUE_OVERFLOW, UB_REVERT_LOOP, UB_BAD_INDEX, UB_FLAME_QUEUE_RANGE = 1, 2, 4, 8, 16, 32
# the reference crashes (or overruns an array) on a tick with one of these: its golden trace ends before such a tick
FATAL = UB_NULL_BOMB | UB_QUEUE_OVERFLOW | UB_REVERT_LOOP | UB_BAD_INDEX

# upload bounds (pom_packed.h POM_PACK_*)
BOMBCOUNT_MIN, BOMBCOUNT_MAX, MAXBOMBS_MAX, STRENGTH_MAX, ALIVE_MIN = -108, 107, 32646, 134, -124


def uploadable(s):
    """the agent fields and aliveAgents within upload's bounds (pom_packed.h POM_PACK_*)"""
    a = s["agents"]
    return bool((a["bombCount"] >= BOMBCOUNT_MIN).all() and (a["bombCount"] <= BOMBCOUNT_MAX).all()
                and (a["maxBombCount"] >= -32768).all() and (a["maxBombCount"] <= MAXBOMBS_MAX).all()
                and (a["bombStrength"] >= 0).all() and (a["bombStrength"] <= STRENGTH_MAX).all()
                and ALIVE_MIN <= int(s["aliveAgents"]) <= 127)


@dataclass
class Entry:
    name: str
    start: np.ndarray  # STATE_DTYPE[1]
    moves: np.ndarray  # int32[T, 4]
    prop: str          # what the entry is about
    expect_ub: int = 0  # flags at least one tick of the oracle's run must raise


def _script(*parts):
    """parts: (Move[4], repeat) pairs -> int32[T, 4]"""
    rows = []
    for mv, k in parts:
        rows += [list(mv)] * k
    return np.array(rows, dtype=np.int32).reshape(-1, 4)


def _idle(k):
    return _script(((I, I, I, I), k))


def _base(corners=True):
    s = S.new_states(1)
    if corners:
        S.put_agents_in_corners(s[0])
    return s


def _flame_cell(x, y):
    return Item.FLAMES + ((x + 11 * y) << 3)


def _queue(s, count, index, head, rest=None, strength=1, seed=0):
    """a hand-built flame queue: `count` entries from slot `index`; the head's timeLeft `head`, the others `rest` (default: head,
    head + 1, ... capped at FLAME_LIFETIME, as a queue built by play has them).  Every live slot gets a flame cell at its origin,
    origins on the inner 9 x 9 cells (the corners' agents are left alone)."""
    rng = np.random.default_rng(seed)
    for k in range(min(count, 20)):
        slot = (index + k) % 20
        x, y = 1 + (k % 9), 2 + (k // 9) * 3
        t = head if k == 0 else (rest if rest is not None else min(head + k, S.FLAME_LIFETIME))
        s["flames_queue"][0, slot] = (x, y, t, strength)
        s["board"][0, y, x] = _flame_cell(x, y)
    s["flames_index"] = index
    s["flames_count"] = count
    # the stale slots hold something other than the defaults
    for k in range(min(count, 20), 20):
        slot = (index + k) % 20
        s["flames_queue"][0, slot] = (int(rng.integers(11)), int(rng.integers(11)), int(rng.integers(-5, 5)), 1)
    return s


def _bombs_on_row(s, y, xs, owner, lives, strength=None):
    """bombs of `owner` on row y with the given lifetimes (cells become BOMB)"""
    if strength is not None:
        s["agents"][0, owner]["bombStrength"] = strength
    for x, life in zip(xs, lives):
        S.plant_bomb(s[0], x, y, owner, set_item=True, life_time=life)


def flame_queue_entries(oracle):
    out = []
    # count x index x head: the table of the issue and around it
    for count in (19, 20, 21, 39, 40, 41, 60, 255):
        for index in (0, 13, 19):
            for head in (-128, -127, -2, -1, 1, 2, 3, 4):
                if count == 255 and head not in (-128, -1, 3, 4):
                    continue
                if count in (19, 20) and index == 19 and head in (-127, 2):
                    continue
                s = _queue(_base(), count, index, head, seed=count * 100 + index)
                ticks = 150 if (count, index) in ((21, 13), (41, 13), (41, 19), (60, 0), (255, 13)) else 24
                out.append(Entry(f"fq_count{count}_index{index}_head{head}", s, _idle(ticks),
                                 "TickFlames / PopFlame on a queue of this length, index and head"))
    # the issue's rows
    s = _queue(_base(), 21, 13, 3, seed=1)
    out.append(Entry("fq_issue_21_head3", s, _idle(160), "head visited twice: 3 -> 1 -> -1, never pops; timeLeft passes -128"))
    s = _queue(_base(), 40, 13, 4, rest=2, seed=2)
    out.append(Entry("fq_issue_40_head4", s, _idle(8), "every slot visited twice: all pop in the reference"))
    s = _queue(_base(), 41, 13, 2, seed=3)
    out.append(Entry("fq_issue_41_head2", s, _idle(150), "head visited three times; timeLeft to -448 in the reference",
                     UB_FLAME_QUEUE_RANGE))
    # 21 flames spawned on one board by SpawnFlame (the 21st overwrites the head's slot)
    s = _base()
    for k in range(21):
        oracle.spawn_flame(s, 1 + k % 9, 1 + 2 * (k // 9), 0)
    out.append(Entry("fq_spawn21", s, _idle(40), "SpawnFlame past 20 entries: NextPos wraps onto the head"))
    s = _base()
    for k in range(45):
        oracle.spawn_flame(s, 1 + k % 9, 1 + (k // 9) * 2, k % 3)
    out.append(Entry("fq_spawn45", s, _idle(40), "SpawnFlame x 45, strengths 0..2"))
    # count passes 255 by explosions while the queue is stuck
    for count, lives in ((250, (1, 2, 3, 4, 5, 6, 7, 8)), (255, (1, 1, 2))):
        s = _queue(_base(), count, 7, -1, rest=-3, seed=count)
        s["agents"][0, 0]["maxBombCount"] = 10
        s["agents"][0, 0]["bombStrength"] = 0
        _bombs_on_row(s, 9, [1 + k for k in range(len(lives))], 0, lives)
        out.append(Entry(f"fq_count{count}_explosions", s, _idle(140),
                         "explosions on a stuck queue: count passes 255 in the reference", UB_FLAME_QUEUE_RANGE))
    # explosions with rays into a stuck queue of 21
    s = _queue(_base(), 21, 13, -1, seed=5)
    s["agents"][0, 1]["maxBombCount"] = 5
    _bombs_on_row(s, 8, (2, 5, 8), 1, (2, 3, 5), strength=2)
    out.append(Entry("fq_stuck21_rays", s, _idle(60), "explosions whose rays cross a stuck queue's flame cells"))
    # a stuck queue of 21 whose agents walk into the flame cells and plant bombs
    s = _queue(_base(), 21, 0, -5, seed=6)
    for a in range(4):
        s["agents"][0, a]["maxBombCount"] = 3
    out.append(Entry("fq_stuck21_agents", s, _script(((B, B, B, B), 1), ((R, L, L, R), 3), ((D, D, U, U), 3), ((I, I, I, I), 40)),
                     "agents plant and walk into a stuck queue's flames"))
    return out


def narrow_field_entries():
    out = []
    # bombCount up: plants while walking along the top row (the bombs go off behind the agent)
    for bc in (BOMBCOUNT_MAX, BOMBCOUNT_MAX - 1):
        s = _base()
        s["agents"][0, 0]["bombCount"] = bc
        s["agents"][0, 0]["maxBombCount"] = 300
        out.append(Entry(f"bombcount_up_{bc}", s, _script(((B, I, I, I), 1), ((R, I, I, I), 1), ((B, I, I, I), 1),
                                                         ((D, I, I, I), 1), ((B, I, I, I), 1), ((D, I, I, I), 1), ((I, I, I, I), 12)),
                         "bombCount grows by plants, shrinks when they go off"))
    # bombCount down: 20 own bombs queued, all go off
    for bc in (BOMBCOUNT_MIN, BOMBCOUNT_MIN + 1):
        s = _base()
        s["agents"][0, 2]["maxBombCount"] = 400
        s["agents"][0, 2]["bombStrength"] = 0
        for k in range(20):
            S.plant_bomb(s[0], 1 + k % 9, 2 + 3 * (k // 9), 2, set_item=True, life_time=1 + k // 4)  # in queue order
        s["agents"][0, 2]["bombCount"] = bc  # bombCount - own queued bombs = bc - 20: where it ends
        out.append(Entry(f"bombcount_down_{bc}", s, _idle(10), "20 own bombs go off: bombCount falls by 20"))
    # maxBombCount: walk over a row of EXTRABOMBs
    for m in (MAXBOMBS_MAX, MAXBOMBS_MAX - 1, -32768):
        s = _base()
        s["agents"][0, 0]["maxBombCount"] = m
        for x in range(1, 10):
            s["board"][0, 0, x] = Item.EXTRABOMB
        out.append(Entry(f"maxbombs_{m}", s, _script(((R, I, I, I), 9), ((B, I, I, I), 1), ((L, I, I, I), 3), ((I, I, I, I), 10)),
                         "maxBombCount grows by pick-ups"))
    # bombStrength: walk over INCRRANGEs, then plant (strength > 15 spills into the bomb's time nibble)
    for st in (STRENGTH_MAX, STRENGTH_MAX - 1, 0):
        s = _base()
        s["agents"][0, 3]["bombStrength"] = st
        s["agents"][0, 3]["maxBombCount"] = 3
        for x in range(1, 8):
            s["board"][0, 10, x] = Item.INCRRANGE
        out.append(Entry(f"strength_{st}", s, _script(((I, I, I, R), 7), ((I, I, I, B), 1), ((I, I, I, U), 4), ((I, I, I, I), 14)),
                         "bombStrength grows by pick-ups; a bomb planted and exploding with it"))
    for st in (15, 16, 17, 31, 32, 100):
        s = _base()
        s["agents"][0, 1]["bombStrength"] = st
        out.append(Entry(f"plant_strength_{st}", s, _script(((I, B, I, I), 1), ((I, D, I, I), 2), ((I, L, I, I), 1), ((I, I, I, I), 14)),
                         "a bomb planted with this strength: the nibble spill and its explosion"))
    # aliveAgents: every agent walks into a flame
    for al in (ALIVE_MIN, ALIVE_MIN + 1, 127):
        s = _base()
        s["aliveAgents"] = al
        for (x, y) in ((1, 0), (9, 0), (9, 10), (1, 10)):
            s["board"][0, y, x] = _flame_cell(x, y)
            k = int(s["flames_count"][0])
            s["flames_queue"][0, k] = (x, y, 3, 0)
            s["flames_count"] = k + 1
        out.append(Entry(f"alive_{al}", s, _script(((R, L, L, R), 1), ((I, I, I, I), 4)), "aliveAgents falls by one per death"))
    # flame timeLeft / strength at the byte's ends
    s = _queue(_base(), 20, 5, -126, rest=-120, strength=255, seed=9)
    out.append(Entry("flame_time_to_minus128", s, _idle(12), "queued timeLeft walks through -128", UB_FLAME_QUEUE_RANGE))
    s = _base()
    for k, (x, y, st) in enumerate(((0, 5, 255), (10, 5, 255), (5, 0, 200), (5, 10, 11), (10, 10, 12))):
        s["board"][0, y, x] = _flame_cell(x, y)
        s["flames_queue"][0, k] = (x, y, 1 + k % 4, st)
    s["board"][0, 0, 0] = Item.PASSAGE  # agents elsewhere: (0, 0) .. corners stay free of flames but (10, 10)
    S.put_agent(s[0], 3, 3, 0)
    S.put_agent(s[0], 7, 3, 1)
    S.put_agent(s[0], 3, 7, 2)
    S.put_agent(s[0], 7, 7, 3)
    s["board"][0, 0, 10] = Item.PASSAGE
    s["board"][0, 10, 0] = Item.PASSAGE
    s["flames_count"] = 5
    out.append(Entry("flame_strength_255_edges", s, _idle(6), "PopFlame's arms of 255 cells from the board's edges"))
    return out


def limit_entries(oracle):
    out = []
    # flagged flame cells 10 cells from their origin: wood with flags 1..4 at the ray's far ends
    for flag in (1, 2, 3, 4):
        s = _base(corners=False)
        S.put_agent(s[0], 5, 5, 0)
        S.put_agent(s[0], 6, 6, 1)
        S.put_agent(s[0], 4, 6, 2)
        S.put_agent(s[0], 6, 4, 3)
        s["board"][0, 0, 10] = Item.WOOD + flag   # 10 cells from (0, 0) along +x
        s["board"][0, 10, 0] = Item.WOOD + flag   # and along +y
        oracle.spawn_flame(s, 0, 0, 10)
        out.append(Entry(f"flagged_10_cells_flag{flag}", s, _script(((I, I, I, I), 6), ((U, I, I, I), 5)),
                         "flagged flame cells 10 cells out pop to their power-up"))
    # wood flags 1..4 under a bomb's rays
    s = _base()
    s["agents"][0, 0]["maxBombCount"] = 2
    s["agents"][0, 0]["bombStrength"] = 3
    for k, flag in enumerate((1, 2, 3, 4)):
        s["board"][0, 5, 3 + 2 * k] = Item.WOOD + flag
    _bombs_on_row(s, 6, (5,), 0, (2,))
    s["board"][0, 4, 5] = Item.WOOD + 4
    s["board"][0, 6, 4] = Item.WOOD + 2
    s["board"][0, 6, 6] = Item.WOOD + 3
    s["board"][0, 7, 5] = Item.WOOD + 1
    out.append(Entry("wood_flags_under_flames", s, _idle(10), "wood flags 1..4 under flames and what they pop to"))
    # a full bomb queue, index 19, taking more plants (the reference overruns an array: POM_UB_QUEUE_OVERFLOW)
    for index in (0, 19):
        s = _base()
        s["bombs_index"] = index
        for a in range(4):
            s["agents"][0, a]["maxBombCount"] = 30
            s["agents"][0, a]["bombStrength"] = 1
        for k in range(20):
            S.plant_bomb(s[0], 2 + k % 7, 2 + 2 * (k // 7), k % 4, set_item=True, life_time=8 + k % 3)
        out.append(Entry(f"bomb_queue_full_index{index}", s, _script(((B, B, B, B), 1), ((D, L, U, R), 1), ((B, B, B, B), 1),
                                                                     ((I, I, I, I), 12)),
                         "a full bomb queue taking more plants", UB_QUEUE_OVERFLOW))
    # NULL_BOMB: a kicker steps onto a BOMB cell that has no queue entry
    s = _base()
    s["agents"][0, 0]["canKick"] = 1
    s["board"][0, 0, 1] = Item.BOMB
    out.append(Entry("ub_null_bomb", s, _script(((R, I, I, I), 1), ((I, I, I, I), 2)), "kick of a ghost BOMB", UB_NULL_BOMB))
    # an explosion's ray over a live flame cell of another origin
    s = _base()
    s["agents"][0, 0]["maxBombCount"] = 2
    s["agents"][0, 0]["bombStrength"] = 2
    _bombs_on_row(s, 5, (5,), 0, (1,))
    s["board"][0, 5, 6] = _flame_cell(6, 5)
    s["flames_queue"][0, 0] = (6, 5, 3, 0)
    s["flames_count"] = 1
    out.append(Entry("ray_over_flame_cell", s, _idle(6), "an explosion's ray over a flame cell"))
    # LOST_AGENT: the reference's "Two On One" shape
    s = _base(corners=False)
    S.put_agent(s[0], 0, 0, 0)
    S.put_agent(s[0], 1, 0, 1)
    S.put_agent(s[0], 2, 0, 2)
    S.put_agent(s[0], 1, 1, 3)
    out.append(Entry("ub_lost_agent", s, _script(((R, R, L, U), 1), ((I, I, I, I), 2)), "three agents for one cell"))
    return out


def corpus(oracle):
    entries = flame_queue_entries(oracle) + narrow_field_entries() + limit_entries(oracle)
    names = [e.name for e in entries]
    assert len(set(names)) == len(names)
    for e in entries:
        e.start["agents"]["pad"] = 0
    return entries
