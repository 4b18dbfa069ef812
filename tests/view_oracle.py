"""TEST INFRASTRUCTURE — the fogged per-agent views (pom_batch.h PomViewSpec) derived from the UNFOGGED outputs of
oracle/pom_observe_oracle.py: mask by the viewer's window, fill fog, build viewer_attrs.  Nothing of the export's own logic is
restated here, so the views are pinned by what the suite already pins."""
import numpy as np

N = 11
FOG = 5  # Item::FOG


def windows(agent_attrs: np.ndarray, radius: int) -> np.ndarray:
    """bool [n, 4, 11, 11]: the cells view v of env e shows — |x - x_v| <= r and |y - y_v| <= r around the position agent_attrs
    reports (alive or dead), clipped by the board"""
    x = agent_attrs[:, :, 0].astype(np.int64)[:, :, None, None]
    y = agent_attrs[:, :, 1].astype(np.int64)[:, :, None, None]
    xs = np.arange(N)[None, None, None, :]
    ys = np.arange(N)[None, None, :, None]
    return (np.abs(xs - x) <= radius) & (np.abs(ys - y) <= radius)


def view_planes(per_agent_planes: np.ndarray, agent_attrs: np.ndarray, radius: int) -> np.ndarray:
    """[n, 4, 16, 11, 11] of observe(states, per_agent=True, dtype): all 16 planes 0 outside the window"""
    assert per_agent_planes.ndim == 5 and per_agent_planes.shape[1:] == (4, 16, N, N)
    w = windows(agent_attrs, radius)[:, :, None]
    return np.where(w, per_agent_planes, np.zeros((), dtype=per_agent_planes.dtype))


def view_codes(codes: np.ndarray, agent_attrs: np.ndarray, radius: int) -> np.ndarray:
    """uint8 [n, 4, 5, 11, 11] of observe_codes(states) [n, 5, 11, 11]: outside the window the board reads fog, the rest 0"""
    assert codes.ndim == 4 and codes.shape[1:] == (5, N, N)
    w = windows(agent_attrs, radius)[:, :, None]
    fog = np.zeros((1, 1, 5, 1, 1), dtype=codes.dtype)
    fog[0, 0, 0] = FOG
    return np.where(w, codes[:, None], fog)


def viewer_attrs(agent_attrs: np.ndarray, time_step: np.ndarray) -> np.ndarray:
    """int32 [n, 4, 12]: the viewer's own row of agent_attrs, the alive flags of agents v+1, v+2, v+3 (mod 4), timeStep"""
    n = len(agent_attrs)
    out = np.zeros((n, 4, 12), dtype=np.int32)
    for v in range(4):
        out[:, v, :8] = agent_attrs[:, v]
        for k in (1, 2, 3):
            out[:, v, 7 + k] = agent_attrs[:, (v + k) % 4, 2]
        out[:, v, 11] = time_step
    return out
