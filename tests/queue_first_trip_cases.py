"""A hand-made corpus for the queue loops every tick runs (pomcpp_amd/csrc/pom_step_body.h: flames_dec, flame_pops, step_middle's
scan of the bombs under agents and its bomb pass) — test infrastructure, in the form of tests/edge_states.py.

With a quad per env, lane `sub` of the quad plays queue offset `sub` straight-line and only offsets 4 and up go through a loop.  The
entries sit on both sides of that seam and where the first trip could take the wrong slot or the wrong lane's word:
  flames  counts 0, 1, 3, 4, 5, 8, 20 and above 20, heads at slots 17 - 19 (the offsets wrap), two flames that run out in one tick,
          arms of length 0 (strength 0; a flame on an edge and in a corner), 1 and 2 and more, a flagged wood flame on an arm's first
          and on its second cell, a timer that reaches -128 and one that is held there;
  bombs   counts 0, 1, 4, 5, 8, 20, heads at slots 17 - 19, a timer of 0 queued behind a later one (`late`), two resting bombs on one
          cell, a bomb under an agent that walked onto it this tick (`cand`), a bomb under an agent who walks off it, a moving bomb at offset 0 and at offset 4, a bomb planted
          this tick into the slot offset 4 reads.

corpus(oracle) is deterministic.  tests/test_queue_first_trip.py plays every entry through the four-lane host model and the one-lane
one; tests/test_gpu_queue_first_trip.py through the kernels, each entry in every column of a tile.
"""
from __future__ import annotations

import numpy as np

import pomcpp_amd.state as S
from pomcpp_amd.state import Item
from tests.edge_states import Entry, _base, _idle, _queue, _script
from tests.edge_states import B, D, I, L, R, U  # noqa: F401
from tests.edge_states import UB_FLAME_QUEUE_RANGE

TICKS = 8  # every entry's script has this many ticks
INNER = ((3, 3), (7, 3), (3, 7), (7, 7))  # where the agents stand when the corners and edges are needed
# flame origins that keep clear of INNER and of each other's first arm cells where it matters (later ones may overlap: their cells
# then carry the later origin, as after play)
ORIGINS = ((1, 1), (5, 1), (9, 1), (1, 5), (5, 5), (9, 5), (1, 9), (5, 9), (9, 9), (0, 3), (10, 3), (0, 7), (10, 7), (3, 0), (7, 0),
           (3, 10), (7, 10), (5, 3), (5, 7), (0, 5))
# bomb cells: the inner columns, clear of INNER and of the rows next to the corners
BOMB_CELLS = tuple((x, y) for y in (1, 5, 9, 2, 8) for x in (1, 5, 9, 2, 8))[:20]


def _inner():
    s = _base(corners=False)
    for a, (x, y) in enumerate(INNER):
        S.put_agent(s[0], x, y, a)
    return s


def _rotate(s, which, index):
    """the queue built from slot 0 moved so that its head sits in slot `index` (stale slots travel along)"""
    q = s[f"{which}_queue"][0].copy()
    for k in range(20):
        s[f"{which}_queue"][0, (index + k) % 20] = q[k]
    s[f"{which}_index"] = index
    return s


def _spawn(oracle, s, flames, index=0):
    """flames: (x, y, strength, timeLeft) in queue order, spawned by SpawnFlame (arms, burnt wood and all), then given their timers"""
    for (x, y, strength, _t) in flames:
        oracle.spawn_flame(s, x, y, strength)
    assert int(s["flames_count"][0]) == len(flames) <= 20
    for k, f in enumerate(flames):
        s["flames_queue"][0, k]["timeLeft"] = f[3]
    return _rotate(s, "flames", index)


def _times(n, first=1):
    """timers as play leaves them: never falling along the queue; the first two run out together"""
    return [min(S.FLAME_LIFETIME, first + k // 2) for k in range(n)]


def flame_entries(oracle):
    out = []
    for n, index in ((0, 18), (1, 19), (1, 0), (3, 18), (4, 17), (4, 0), (5, 19), (5, 0), (8, 17), (8, 18), (20, 19), (20, 17)):
        flames = [(x, y, 1, t) for (x, y), t in zip(ORIGINS[:n], _times(n))]
        out.append(Entry(f"fl_count{n}_head{index}", _spawn(oracle, _inner(), flames, index), _idle(TICKS),
                         f"{n} flames from slot {index}: two run out per tick"))
    # nothing pops: the head still has time (the first trip's early way out), five and eight queued
    for n, index in ((5, 18), (8, 19)):
        flames = [(x, y, 1, 4) for (x, y) in ORIGINS[:n]]
        out.append(Entry(f"fl_count{n}_head{index}_young", _spawn(oracle, _inner(), flames, index), _idle(TICKS), "no pop for three ticks"))
    # more than 20 queued: every slot visited once per offset, the head more than once (tests/edge_states.py builds these)
    for count, index, head in ((21, 17, 3), (21, 19, 1), (23, 18, 2), (41, 19, 4)):
        s = _queue(_base(), count, index, head, seed=count + index)
        out.append(Entry(f"fl_count{count}_head{index}_time{head}", s, _idle(TICKS), "a queue of more than 20: the head's slot is visited again"))
    # arms: strength 0 (no arm at all), an edge and a corner (arms of length 0 off the board), 1, 2, 3; two flames run out together
    arms = [(0, 0, 2, 1), (10, 10, 3, 1), (5, 0, 2, 2), (0, 5, 1, 2), (10, 6, 2, 3), (5, 10, 3, 3), (5, 5, 0, 4), (8, 5, 3, 4)]
    for index in (0, 17):
        out.append(Entry(f"fl_arms_head{index}", _spawn(oracle, _inner(), arms, index), _idle(TICKS), "arms of length 0, 1, 2 and 3"))
    # flagged wood flames: wood with a power-up on an arm's first cell (flags 1, 2, 3, one per direction) and on its second
    for where, dist in (("first", 1), ("second", 2)):
        s = _inner()
        for (x, y), (dx, dy), flag in (((5, 5), (1, 0), 1), ((5, 5), (-1, 0), 2), ((5, 5), (0, 1), 3), ((5, 5), (0, -1), 1),
                                         ((1, 1), (1, 0), 2), ((1, 1), (0, 1), 3), ((9, 9), (-1, 0), 3), ((9, 9), (0, -1), 4)):
            s["board"][0, y + dy * dist, x + dx * dist] = Item.WOOD + flag
        flames = [(5, 5, 2, 1), (1, 1, 3, 1), (9, 9, 2, 2)]
        out.append(Entry(f"fl_flagged_{where}_cell", _spawn(oracle, s, flames, 19), _idle(TICKS),
                         f"flagged wood flames on the {where} cell of an arm pop to their power-ups"))
    # timers at the record's lower end: -127 reaches -128 (still the reference's value), then it is held; held from the start; at the
    # head, at offset 3 and at offset 5 (behind the first trip)
    for name, at, t in (("reaches", 0, -127), ("held", 0, -128), ("held", 3, -128), ("held", 5, -128), ("reaches", 5, -127)):
        flames = [(x, y, 1, 4) for (x, y) in ORIGINS[:7]]
        s = _spawn(oracle, _inner(), flames, 18)
        for k in range(7):
            s["flames_queue"][0, (18 + k) % 20]["timeLeft"] = -100 + k  # a stuck queue: nothing pops
        s["flames_queue"][0, (18 + at) % 20]["timeLeft"] = t
        out.append(Entry(f"fl_minus128_{name}_offset{at}", s, _idle(TICKS), "timeLeft at -128", UB_FLAME_QUEUE_RANGE))
    return out


def _bombers(s, n=30, strength=1):
    for a in range(4):
        s["agents"][0, a]["maxBombCount"] = n
        s["agents"][0, a]["bombStrength"] = strength


def _bombs(s, n, index=0, lives=None, cells=BOMB_CELLS):
    """n resting bombs in queue order from slot `index`, owners in rotation; lives default to 9, 9, 10, 10, ... (never falling)"""
    s["bombs_index"] = index
    for k in range(n):
        x, y = cells[k]
        S.plant_bomb(s[0], x, y, k % 4, set_item=True, life_time=(lives[k] if lives else min(10, 9 + k // 2)))
    assert int(s["bombs_count"][0]) == n
    return s


def bomb_entries():
    out = []
    walk = _script(((R, L, L, R), 1), ((D, D, U, U), 1), ((I, I, I, I), TICKS - 2))
    for n, index in ((0, 17), (1, 18), (1, 0), (4, 19), (4, 0), (5, 17), (5, 0), (8, 18), (8, 19), (20, 17), (20, 19), (20, 0)):
        s = _base()
        _bombers(s)
        out.append(Entry(f"bo_count{n}_head{index}", _bombs(s, n, index), walk, f"{n} resting bombs from slot {index}"))
    # the head and its followers go off: timers 1, 1, 2, 2, ... (top_explosions takes the head the pass hands it)
    for n, index in ((5, 19), (8, 17)):
        s = _base()
        _bombers(s)
        out.append(Entry(f"bo_count{n}_head{index}_ripe", _bombs(s, n, index, lives=[1 + k // 2 for k in range(n)]), _idle(TICKS),
                         "bombs going off two per tick from the head"))
    # `late`: a timer of 0 queued behind a later one, at offset 1 (first trip) and at offset 5 (the loop behind it)
    for at in (1, 5):
        s = _base()
        _bombers(s)
        lives = [6] * 8
        lives[at] = 0
        out.append(Entry(f"bo_late_offset{at}", _bombs(s, 8, 18, lives=lives), _idle(TICKS), "a timer of 0 behind a later one: decremented after loop B"))
    # two resting bombs on one cell: offsets 0 and 1; offsets 3 and 4 (either side of the seam)
    for a, b2 in ((0, 1), (3, 4)):
        s = _base()
        _bombers(s)
        cells = list(BOMB_CELLS)
        cells[b2] = cells[a]
        out.append(Entry(f"bo_shared_cell_{a}_{b2}", _bombs(s, 6, 19, cells=cells, lives=[3, 3, 4, 4, 5, 5]), _idle(TICKS), "two resting bombs on one cell"))
    # `cand`: an agent walks onto a resting bomb this tick and is bounced back — the bomb at offset 0, 3, 4 and 7
    for at in (0, 3, 4, 7):
        s = _base(corners=False)
        S.put_agent(s[0], 4, 5, 0)
        for a, (x, y) in ((1, (10, 0)), (2, (10, 10)), (3, (0, 10))):
            S.put_agent(s[0], x, y, a)
        _bombers(s)
        cells = [c for c in BOMB_CELLS if c != (5, 5)]
        cells.insert(at, (5, 5))
        out.append(Entry(f"bo_walked_onto_offset{at}", _bombs(s, 8, 17, cells=cells), _script(((R, I, I, I), 2), ((I, I, I, I), TICKS - 2)),
                         "an agent steps onto a resting bomb: bounced back in loop A"))
    # the scan of the bombs under agents: an agent stands on a queued bomb (offset 0, 3, 4, 7) and walks off — the cell he leaves shows BOMB
    for at in (0, 3, 4, 7):
        s = _base(corners=False)
        _bombers(s)
        cells = [c for c in BOMB_CELLS if c != (5, 5)]
        cells.insert(at, (5, 5))
        _bombs(s, 8, 19, cells=cells)
        S.put_agent(s[0], 5, 5, 1)
        for a, (x, y) in ((0, (0, 0)), (2, (10, 10)), (3, (0, 10))):
            S.put_agent(s[0], x, y, a)
        out.append(Entry(f"bo_left_behind_offset{at}", s, _script(((I, R, I, I), 1), ((I, I, I, I), TICKS - 1)), "an agent walks off the bomb he stands on"))
    # a moving bomb at offset 0 and at offset 4 (and a kicker that sets one moving at offset 5)
    for at in (0, 4):
        s = _base()
        _bombers(s)
        _bombs(s, 6, 18)
        S.set_bomb_direction(s[0], at, 2 if BOMB_CELLS[at][1] < 5 else 1)
        out.append(Entry(f"bo_moving_offset{at}", s, _idle(TICKS), "a bomb with a direction: the literal loops A and B"))
    s = _base(corners=False)
    S.put_agent(s[0], 8, 5, 0)
    for a, (x, y) in ((1, (10, 0)), (2, (10, 10)), (3, (0, 10))):
        S.put_agent(s[0], x, y, a)
    _bombers(s)
    s["agents"][0, 0]["canKick"] = 1
    cells = [c for c in BOMB_CELLS if c != (9, 5)]
    cells.insert(5, (7, 5))
    out.append(Entry("bo_kicked_offset5", _bombs(s, 7, 19, cells=cells), _script(((L, I, I, I), 1), ((I, I, I, I), TICKS - 1)), "a kick sets offset 5 moving"))
    # planted this tick into the slot offset 4 reads (and offsets 1, 5: either side), stale bits in the slot; all four plant at once
    for have, index in ((4, 17), (1, 19), (5, 18), (3, 19)):
        s = _base()
        _bombers(s)
        _bombs(s, have, index)
        for k in range(have, 20):  # stale words with a direction and flags in the free slots (they survive a plant)
            s["bombs_queue"][0, (index + k) % 20] = S._i32(0x01300000 | ((k % 11) << 4) | 0xA)
        moves = _script(((B, I, I, I), 1), ((R, I, I, I), 1), ((I, B, I, I), 1), ((B, B, B, B), 1), ((I, I, I, I), TICKS - 4))
        out.append(Entry(f"bo_planted_into_offset{have}_head{index}", s, moves, f"a bomb planted this tick into offset {have}"))
    return out


def corpus(oracle):
    entries = flame_entries(oracle) + bomb_entries()
    names = [e.name for e in entries]
    assert len(set(names)) == len(names)
    for e in entries:
        e.start["agents"]["pad"] = 0
        assert e.moves.shape == (TICKS, 4), e.name
    return entries


def traces(oracle, entries):
    """the oracle's run of every entry alone: states uint8[E, TICKS, 1004] as the record holds them, the ticks' flags uint32[E, TICKS].
    A flame timer below -128 does not fit the record, which holds it at -128 from the tick that raises POM_UB_FLAME_QUEUE_RANGE on
    (include/pom_state.h; the reference's value only falls further and nothing else can tell): the expected state has it there"""
    states = np.zeros((len(entries), TICKS, 1004), dtype=np.uint8)
    ubs = np.zeros((len(entries), TICKS), dtype=np.uint32)
    for i, e in enumerate(entries):
        s = e.start.copy()
        for t in range(TICKS):
            ubs[i, t] = oracle.step(s, e.moves[t])
            s["agents"]["pad"] = 0
            w = s.copy()
            w["flames_queue"]["timeLeft"] = np.maximum(w["flames_queue"]["timeLeft"], -128)
            states[i, t] = np.frombuffer(w.tobytes(), dtype=np.uint8)
    return states, ubs
