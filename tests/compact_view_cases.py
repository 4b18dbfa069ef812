"""TEST INFRASTRUCTURE — hand-made states for the compact views (pom_batch.h PomCompactViewSpec): viewers in all four corners, on each
edge, in the middle, and a dead one; every cell of the boards holds something a crop can be told by."""
import functools

import numpy as np

from pomcpp_amd.state import Item, new_states

# (x, y, dead) of the four agents of each hand-made env
PLACES = [
    [(0, 0, 0), (10, 0, 0), (0, 10, 0), (10, 10, 0)],   # the four corners
    [(5, 0, 0), (0, 5, 0), (10, 5, 0), (5, 10, 0)],     # the four edges
    [(5, 5, 0), (3, 7, 0), (10, 3, 1), (8, 9, 0)],      # the middle, off-centre, a dead viewer on the right edge, near a corner
]


@functools.lru_cache(maxsize=None)
def hand_states() -> np.ndarray:
    """the three envs of PLACES.  The cells hold a fixed scatter of passage, rigid, wood and the three power-ups; env 2 also a bomb
    and a flame two cells from the viewer in the middle.  Read only (shared)."""
    s = new_states(len(PLACES))
    rng = np.random.default_rng(20261021)
    things = np.array([Item.PASSAGE, Item.PASSAGE, Item.RIGID, Item.WOOD, Item.EXTRABOMB, Item.INCRRANGE, Item.KICK])
    for e, places in enumerate(PLACES):
        b = s["board"][e]                                             # [y][x]
        b[:, :] = things[rng.integers(0, len(things), size=(11, 11))]
        for i, (x, y, dead) in enumerate(places):
            s["agents"][e, i]["x"], s["agents"][e, i]["y"], s["agents"][e, i]["dead"] = x, y, dead
            b[y, x] = Item.PASSAGE if dead else Item.AGENT0 + i
        s["aliveAgents"][e] = sum(1 for p in places if not p[2])
        s["timeStep"][e] = 17 + e
    b = s["board"][2]
    b[5, 7] = Item.BOMB
    s["bombs_queue"][2, 0] = 7 + (5 << 4) + (1 << 8) + (3 << 12) + (6 << 16)
    s["bombs_count"][2] = 1
    s["agents"][2, 1]["bombCount"], s["agents"][2, 1]["maxBombCount"] = 1, 2
    b[3, 5] = Item.FLAMES + ((5 + 11 * 3) << 3)
    s["flames_queue"][2, 0]["x"], s["flames_queue"][2, 0]["y"], s["flames_queue"][2, 0]["timeLeft"] = 5, 3, 2
    s["flames_count"][2] = 1
    s.setflags(write=False)
    return s
