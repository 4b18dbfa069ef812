"""The hand-made States of pom_batch_reach's fixture (tests/golden/reach.npz, tests/golden/gen_reach.py): built cell by cell on a
fresh State, never through the reference's InitBoardItems.  Each is (name, STATE_DTYPE[1]).  Agents that a case does not place are
dead and not on the board.  What the cases are for is said where they are built; tests/test_reach_host.py checks that the fixture
holds them as they are built here."""
import numpy as np

from pomcpp_amd.state import Item, kill, new_states, plant_bomb, put_agent

N = 11


def blank(agents: dict, fill=Item.PASSAGE):
    """a board of `fill` with the agents {id: (x, y)} on it, the others dead"""
    s = new_states(1)
    s["board"][0][:] = fill
    for a in range(4):
        if a in agents:
            put_agent(s[0], agents[a][0], agents[a][1], a)
        else:
            kill(s[0], a)
    return s


def _open(s, cells, item=Item.PASSAGE):
    for x, y in cells:
        s["board"][0, y, x] = item


def empty_board():
    """ties everywhere, and the guards that keep the source at 0: the source in each corner, on each edge, in the centre — every
    agent id takes its turn as the source"""
    spots = [(0, 0), (10, 0), (0, 10), (10, 10), (5, 0), (0, 5), (10, 5), (5, 10), (5, 5)]
    return [(f"empty_{x}_{y}", blank({i % 4: (x, y)})) for i, (x, y) in enumerate(spots)]


def word_boundaries():
    """paths across the boundaries of the 32-cell words (cells 31|32, 63|64, 95|96) along a row and along a column, from either end,
    through rigid boards; and the two leaks a wrong column mask would open: from x = 10 into x = 0 of the next row (cell + 1) and from
    x = 0 into x = 10 of the row before (cell - 1)"""
    out = []
    for b in (32, 64, 96):
        y, x = divmod(b, N)  # cell b; cell b - 1 is its left neighbour (b is never at x = 0)
        for side, sx in (("l", 0), ("r", 10)):
            s = blank({0: (sx, y)}, Item.RIGID)
            _open(s, [(i, y) for i in range(N) if i != sx])
            out.append((f"row_across_{b}_{side}", s))
        # a column through cell b - 1 and one through cell b: both cross from the word before into b's word, or out of it
        for cx in (x - 1, x):
            for side, sy in (("t", 0), ("b", 10)):
                s = blank({1: (cx, sy)}, Item.RIGID)
                _open(s, [(cx, i) for i in range(N) if i != sy])
                out.append((f"col_{cx}_across_{b}_{side}", s))
    # even rows open but for one end cell, odd rows rigid but for both end cells: one end cell connects the even rows, the other is
    # an island that only a shift across the board's edge reaches
    for name, island in (("leak_plus_1", 0), ("leak_minus_1", 10)):
        link = 10 - island
        s = blank({2: (5, 0)}, Item.RIGID)
        for y in range(N):
            if y % 2 == 0:
                _open(s, [(x, y) for x in range(N) if x != island and (x, y) != (5, 0)])
            else:
                _open(s, [(island, y), (link, y)])
        out.append((name, s))
    return out


def long_path():
    """a serpentine: rows 0, 2, .. 10 open, rows 1, 3, .. 9 rigid but for one end cell, alternating; from (0, 0) the far end (0, 10)
    is 70 steps away — a distance that needs the seventh bit"""
    s = blank({0: (0, 0)}, Item.RIGID)
    for y in range(N):
        if y % 2 == 0:
            _open(s, [(x, y) for x in range(N) if (x, y) != (0, 0)])
        else:
            _open(s, [(10 if y % 4 == 1 else 0, y)])
    return [("serpentine", s)]


def blocking_agent():
    """a corridor with an agent in it: its cell is reached, the cells behind it are not — seen from both agents"""
    s = blank({0: (0, 5), 1: (4, 5)}, Item.RIGID)
    _open(s, [(x, 5) for x in range(N) if x not in (0, 4)])
    return [("agent_in_corridor", s)]


def _plus(agents):
    """a rigid board with row 5 and column 5 open: four arms from the centre"""
    s = blank(agents, Item.RIGID)
    taken = set(agents.values())
    _open(s, [c for c in [(x, 5) for x in range(N)] + [(5, y) for y in range(N)] if c not in taken])
    return s


def blockers_and_walkables():
    """the source standing on its own bomb (the board shows the agent) with one blocker in each arm, two cells away: a bomb, wood
    without and with a power-up flag, a flame; then the same arms with what is walked through: the three power-ups — and a flame that
    hides a power-up, which blocks like any flame"""
    a = _plus({0: (5, 5), 1: (0, 0)})
    plant_bomb(a[0], 5, 5, 0)
    plant_bomb(a[0], 7, 5, 1, set_item=True)
    _open(a, [(3, 5)], Item.WOOD)
    _open(a, [(5, 3)], Item.WOOD + 2)
    _open(a, [(5, 7)], Item.FLAMES + ((7 * N + 5) << 3))
    b = _plus({3: (5, 5)})
    _open(b, [(7, 5)], Item.EXTRABOMB)
    _open(b, [(3, 5)], Item.INCRRANGE)
    _open(b, [(5, 3)], Item.KICK)
    _open(b, [(5, 7)], Item.FLAMES + ((5 * N + 5) << 3) + 1)  # origin (5, 5), two cells up the column
    return [("blockers", a), ("walkables", b)]


def dead_agents():
    """one, two and three agents dead (off the board, as a game leaves them) on a board with a few walls"""
    out = []
    spots = {0: (1, 1), 1: (9, 1), 2: (9, 9), 3: (1, 9)}
    for dead in ((2,), (0, 3), (0, 1, 2)):
        s = blank({a: p for a, p in spots.items() if a not in dead})
        _open(s, [(5, y) for y in range(2, 9)] + [(x, 5) for x in range(2, 9)], Item.RIGID)
        out.append(("dead_" + "".join(map(str, dead)), s))
    return out


def hand_made():
    cases = empty_board() + word_boundaries() + long_path() + blocking_agent() + blockers_and_walkables() + dead_agents()
    assert len({n for n, _ in cases}) == len(cases)
    return cases


def fill_rmap(oracle, states):
    """(map121, move_to121) int32 [n, 4, 121] of the oracle's restatement (pom_oracle_fill_rmap, oracle/pom_policy_oracle.c), which
    tests/test_policy_fixtures.py and tests/test_reach_host.py pin to the compiled reference"""
    import ctypes as C
    lib = oracle.lib
    lib.pom_oracle_fill_rmap.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.pom_oracle_fill_rmap.restype = None
    states = np.ascontiguousarray(states)
    n = states.size
    m, mt = np.zeros((n, 4, 121), dtype=np.int32), np.zeros((n, 4, 121), dtype=np.int32)
    base = states.ctypes.data
    for e in range(n):
        for a in range(4):
            lib.pom_oracle_fill_rmap(base + 1004 * e, a, m[e, a].ctypes.data, mt[e, a].ctypes.data)
    return m, mt


def expected_planes(states, map121, move_to121, max_dist: int = 120):
    """what pom_batch_reach must write for the fixture's raw maps (ref_fill_rmap: distance | predecessor << 16 per cell; the Move
    towards every reached cell, -1 elsewhere): (dist, move) uint8 [S, 4, 11, 11] — the distance where it is <= max_dist, the Move
    where that is not 0, and nothing at all for a dead agent"""
    d = (np.asarray(map121) & 0xFFFF).astype(np.int64)
    alive = (states["agents"]["dead"] == 0)[:, :, None]
    keep = (d <= max_dist) & (d != 0) & alive
    dist = np.where(keep, d, 0).astype(np.uint8)
    move = np.where(keep, np.asarray(move_to121), 0).astype(np.uint8)
    return dist.reshape(-1, 4, N, N), move.reshape(-1, 4, N, N)
