"""The hand-made cases of pom_batch_remember_view (include/pom_batch.h PomMemorySpec, THE RULE): each a sequence of two to four frames —
the State a call sees, with its timeStep and episode counter — built cell by cell on a blank board, one per clause of the rule, with
the bytes the rule must leave reasoned by hand in `expect` (cell (x, y) of view v after the k-th call = six bytes: board, bomb strength,
life, direction, flame life, age).  Nothing is stepped: what lies outside a window is by definition not looked at, so a frame only has
to show the window what the case is about.  Agents a case does not place are dead and off the board."""
import numpy as np

from pomcpp_amd.state import Item, kill, plant_bomb, put_agent
from tests.reach_cases import blank

FOG, NEVER = 5, 255
UNSEEN = [FOG, 0, 0, 0, 0, NEVER]


def _bomb_at(s, x, y):
    q, i0, cnt = s["bombs_queue"], int(s["bombs_index"]), int(s["bombs_count"])
    return any((int(q[(i0 + k) % 20]) & 0xFF) == x + (y << 4) for k in range(cnt))


def at(s, t, moves=None, dead=(), edit=None):
    """a copy of the one-State array `s` at timeStep t: the agents of `moves` {id: (x, y)} walked there (the cell they leave shows the
    bomb lying on it, or passage), those of `dead` killed and taken off the board, then `edit(state)`"""
    s = s.copy()
    st = s[0]
    st["timeStep"] = t
    for a, (x, y) in (moves or {}).items():
        ox, oy = int(st["agents"][a]["x"]), int(st["agents"][a]["y"])
        st["board"][oy, ox] = Item.BOMB if _bomb_at(st, ox, oy) else Item.PASSAGE
        put_agent(st, x, y, a)
    for a in dead:
        ox, oy = int(st["agents"][a]["x"]), int(st["agents"][a]["y"])
        if st["board"][oy, ox] == Item.AGENT0 + a:
            st["board"][oy, ox] = Item.PASSAGE
        kill(st, a)
    if edit:
        edit(st)
    return s


def put_flame(st, x, y, life):
    """one flame cell, its own centre, with `life` ticks left"""
    k = (int(st["flames_index"]) + int(st["flames_count"])) % 20
    st["flames_queue"][k] = (x, y, life, 0)
    st["flames_count"] += 1
    st["board"][y, x] = Item.FLAMES + ((x + 11 * y) << 3)


def _case(name, radius, frames, expect, mask=1):
    """frames: [(state, episode)]; expect: [(call k, view v, x, y, six bytes)]"""
    return dict(name=name, radius=radius, mask=mask, frames=frames, expect=expect)


def cases():
    out = []
    # a bomb that runs out while unseen: seen with life 3 at t = 10; two ticks later the viewer has walked off (life 1, still a bomb),
    # one more and it is forgotten
    s = blank({0: (1, 1), 1: (9, 9)})
    plant_bomb(s[0], 2, 2, 1, set_item=True, life_time=3)
    s = at(s, 10)
    away = at(s, 12, {0: (5, 1)})
    out.append(_case("bomb_runs_out_unseen", 1, [(s, 0), (away, 0), (at(away, 13), 0)],
                     [(0, 0, 2, 2, [3, 1, 3, 0, 0, 0]), (1, 0, 2, 2, [3, 1, 1, 0, 0, 2]), (2, 0, 2, 2, [0, 0, 0, 0, 0, 3]),
                      (2, 0, 1, 1, [0, 0, 0, 0, 0, 3])]))   # (and the viewer's own trail: it is never believed to be where it was)
    # ... under a remembered agent: agent 1 stands on its bomb (the board shows the agent, the bomb planes the bomb).  The bomb runs out, the
    # agent code stays; then agent 1 is seen elsewhere and the cell is passage
    s = blank({0: (1, 1), 1: (2, 2)})
    plant_bomb(s[0], 2, 2, 1, life_time=2)
    s = at(s, 20)
    f1 = at(s, 21, {0: (5, 1)})
    f3 = at(f1, 23, {1: (5, 2)})
    out.append(_case("bomb_runs_out_under_agent", 1, [(s, 0), (f1, 0), (at(f1, 22), 0), (f3, 0)],
                     [(0, 0, 2, 2, [11, 1, 2, 0, 0, 0]), (1, 0, 2, 2, [11, 1, 1, 0, 0, 1]), (2, 0, 2, 2, [11, 0, 0, 0, 0, 2]),
                      (3, 0, 2, 2, [0, 0, 0, 0, 0, 3]), (3, 0, 5, 2, [11, 0, 0, 0, 0, 0])]))
    # a stale agent leaves the bomb it stood on while that still ticks: the cell becomes a bomb, not passage
    s = blank({0: (1, 1), 1: (2, 2)})
    plant_bomb(s[0], 2, 2, 1, life_time=5)
    s = at(s, 20)
    out.append(_case("stale_agent_leaves_its_bomb", 1, [(s, 0), (at(s, 22, {0: (5, 1), 1: (6, 2)}), 0)],
                     [(0, 0, 2, 2, [11, 1, 5, 0, 0, 0]), (1, 0, 2, 2, [3, 1, 3, 0, 0, 2]), (1, 0, 6, 2, [11, 0, 0, 0, 0, 0])]))
    # a flame that runs out
    s = at(blank({0: (1, 1)}), 5, edit=lambda st: put_flame(st, 2, 1, 3))
    away = at(s, 7, {0: (1, 5)})
    out.append(_case("flame_runs_out", 1, [(s, 0), (away, 0), (at(away, 8), 0)],
                     [(0, 0, 2, 1, [4, 0, 0, 0, 3, 0]), (1, 0, 2, 1, [4, 0, 0, 0, 1, 2]), (2, 0, 2, 1, [0, 0, 0, 0, 0, 3])]))
    # an enemy remembered, then seen elsewhere; another remembered, then dead
    s = at(blank({0: (2, 2), 1: (3, 3), 2: (3, 1)}), 30)
    f1 = at(s, 31, {0: (8, 8)})
    f2 = at(f1, 32, {1: (7, 7)})
    f3 = at(f2, 33, dead=(2,))
    out.append(_case("enemy_remembered_seen_elsewhere_dead", 2, [(s, 0), (f1, 0), (f2, 0), (f3, 0)],
                     [(0, 0, 3, 3, [11, 0, 0, 0, 0, 0]), (1, 0, 3, 3, [11, 0, 0, 0, 0, 1]), (1, 0, 3, 1, [12, 0, 0, 0, 0, 1]),
                      (2, 0, 3, 3, [0, 0, 0, 0, 0, 2]), (2, 0, 7, 7, [11, 0, 0, 0, 0, 0]), (2, 0, 3, 1, [12, 0, 0, 0, 0, 2]),
                      (3, 0, 3, 1, [0, 0, 0, 0, 0, 3]), (3, 0, 7, 7, [11, 0, 0, 0, 0, 0])]))
    # the viewer's own trail at radius 0: it sees one cell, and never remembers itself where it was
    s = at(blank({0: (4, 4)}), 0)
    f1 = at(s, 1, {0: (5, 4)})
    f2 = at(f1, 2, {0: (6, 4)})
    out.append(_case("own_trail_radius_0", 0, [(s, 0), (f1, 0), (f2, 0)],
                     [(0, 0, 4, 4, [10, 0, 0, 0, 0, 0]), (0, 0, 5, 4, UNSEEN), (1, 0, 4, 4, [0, 0, 0, 0, 0, 1]), (2, 0, 4, 4, [0, 0, 0, 0, 0, 2]),
                      (2, 0, 5, 4, [0, 0, 0, 0, 0, 1]), (2, 0, 6, 4, [10, 0, 0, 0, 0, 0]), (2, 0, 7, 4, UNSEEN)]))
    # a dead viewer looks out from where it died: its window goes on being copied
    s = at(blank({0: (3, 3), 1: (9, 9)}), 40, edit=lambda st: st["board"].__setitem__((4, 4), Item.EXTRABOMB))
    f1 = at(s, 41, dead=(0,), edit=lambda st: st["board"].__setitem__((4, 4), Item.PASSAGE))
    out.append(_case("dead_viewer", 1, [(s, 0), (f1, 0)],
                     [(0, 0, 3, 3, [10, 0, 0, 0, 0, 0]), (0, 0, 4, 4, [6, 0, 0, 0, 0, 0]), (1, 0, 3, 3, [0, 0, 0, 0, 0, 0]),
                      (1, 0, 4, 4, [0, 0, 0, 0, 0, 0]), (1, 0, 9, 9, UNSEEN)]))
    # the age saturates at 254 (and dt at 255); a cell never seen stays 255 and fog whatever time passes
    s = at(blank({0: (0, 0)}), 0)
    f1 = at(s, 100, {0: (1, 0)})
    f2 = at(f1, 400)
    out.append(_case("age_saturates_never_seen_stays", 0, [(s, 0), (f1, 0), (f2, 0), (at(f2, 401), 0)],
                     [(1, 0, 0, 0, [0, 0, 0, 0, 0, 100]), (2, 0, 0, 0, [0, 0, 0, 0, 0, 254]), (3, 0, 0, 0, [0, 0, 0, 0, 0, 254]),
                      (3, 0, 1, 0, [10, 0, 0, 0, 0, 0]), (3, 0, 10, 10, UNSEEN), (3, 0, 2, 0, UNSEEN)]))
    # the wipe on a new episode, and on t < t0: what was seen in the old game is gone, the window is the new board's
    s = at(blank({0: (1, 1)}), 50, edit=lambda st: st["board"].__setitem__((2, 2), Item.WOOD))
    new_game = at(blank({0: (8, 8)}), 0)
    out.append(_case("wipe_on_new_episode", 1, [(s, 0), (new_game, 1)],
                     [(0, 0, 2, 2, [2, 0, 0, 0, 0, 0]), (1, 0, 2, 2, UNSEEN), (1, 0, 1, 1, UNSEEN), (1, 0, 8, 8, [10, 0, 0, 0, 0, 0])]))
    out.append(_case("wipe_on_earlier_time_step", 1, [(s, 3), (at(s, 20, {0: (8, 8)}), 3)],
                     [(0, 0, 2, 2, [2, 0, 0, 0, 0, 0]), (1, 0, 2, 2, UNSEEN), (1, 0, 1, 1, UNSEEN), (1, 0, 8, 8, [10, 0, 0, 0, 0, 0])]))
    # dt = 0: a second call at the same tick changes nothing — not even a remembered flame whose life reads 0, or the wood
    s = blank({0: (1, 1), 1: (9, 9)})
    plant_bomb(s[0], 2, 2, 1, set_item=True, life_time=9)
    s = at(s, 10, edit=lambda st: (put_flame(st, 2, 1, 0), st["board"].__setitem__((0, 0), Item.WOOD + 2)))
    away = at(s, 13, {0: (5, 5)})
    out.append(_case("dt_0", 1, [(s, 0), (at(s, 10, {0: (5, 5)}), 0), (away, 0), (away, 0)],
                     [(0, 0, 2, 1, [4, 0, 0, 0, 0, 0]), (1, 0, 2, 1, [4, 0, 0, 0, 0, 0]), (1, 0, 1, 1, [10, 0, 0, 0, 0, 0]), (1, 0, 2, 2, [3, 1, 9, 0, 0, 0]),
                      (2, 0, 2, 1, [0, 0, 0, 0, 0, 3]), (2, 0, 1, 1, [0, 0, 0, 0, 0, 3]), (2, 0, 2, 2, [3, 1, 6, 0, 0, 3]), (2, 0, 0, 0, [2, 0, 0, 0, 0, 3]),
                      (3, 0, 2, 1, [0, 0, 0, 0, 0, 3]), (3, 0, 2, 2, [3, 1, 6, 0, 0, 3]), (3, 0, 0, 0, [2, 0, 0, 0, 0, 3]), (3, 0, 5, 5, [10, 0, 0, 0, 0, 0])]))
    # dt = 3: a call every third tick ages by three
    out.append(_case("dt_3", 1, [(s, 0), (away, 0), (at(away, 16), 0), (at(away, 19), 0), (at(away, 22), 0)],
                     [(1, 0, 2, 2, [3, 1, 6, 0, 0, 3]), (2, 0, 2, 2, [3, 1, 3, 0, 0, 6]), (3, 0, 2, 2, [0, 0, 0, 0, 0, 9]), (4, 0, 2, 2, [0, 0, 0, 0, 0, 12]),
                      (4, 0, 0, 0, [2, 0, 0, 0, 0, 12])]))
    # a window clipped at a corner: two viewers in opposite corners, radius 4 — 25 cells each
    s = at(blank({0: (0, 0), 3: (10, 10)}), 7)
    out.append(_case("window_clipped_at_a_corner", 4, [(s, 0), (at(s, 8), 0)],
                     [(1, 0, 0, 0, [10, 0, 0, 0, 0, 0]), (1, 0, 4, 4, [0, 0, 0, 0, 0, 0]), (1, 0, 5, 4, UNSEEN), (1, 0, 4, 5, UNSEEN), (1, 0, 10, 10, UNSEEN),
                      (1, 3, 10, 10, [13, 0, 0, 0, 0, 0]), (1, 3, 6, 6, [0, 0, 0, 0, 0, 0]), (1, 3, 5, 6, UNSEEN), (1, 3, 0, 0, UNSEEN),
                      (1, 1, 0, 0, [0xEE] * 6)], mask=0b1001))   # (a view outside the mask keeps the test's sentinel)
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


def inputs_of(obs, state, episode):
    """what the checker and the host build take of one frame: (codes [1, 5, 11, 11], agent_attrs [1, 4, 8], env_attrs [1, 4], episodes
    [1]); obs: oracle/pom_observe_oracle.py"""
    _, attrs, env2 = obs.observe(state)
    env = np.zeros((1, 4), dtype=np.int32)
    env[:, :2] = env2
    return obs.observe_codes(state), attrs, env, np.array([episode], dtype=np.uint32)
