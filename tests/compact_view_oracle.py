"""TEST INFRASTRUCTURE — the compact views (pom_batch.h PomCompactViewSpec) derived from the four-view arrays of tests/view_oracle.py
(or of the four-view kernel): rows selected by the mask, and for the centred form each view cut out of itself around the viewer, with
what lies off the board filled in.  An index shuffle; nothing of the kernel is restated."""
import numpy as np

N = 11
FOG = 5  # Item::FOG


def viewers_of(mask: int) -> list:
    """the chosen viewers v_0 < .. < v_{k-1}"""
    assert 1 <= mask <= 15
    return [v for v in range(4) if (mask >> v) & 1]


def side(radius: int, centred: bool) -> int:
    return 2 * radius + 1 if centred else N


def compact_codes(view_codes: np.ndarray, agent_attrs: np.ndarray, radius: int, mask: int, centred: bool) -> np.ndarray:
    """uint8 [n, k, 5, S, S] of the four-view array uint8 [n, 4, 5, 11, 11] written for the same states and radius.  agent_attrs: any
    int array [n, 4, >= 2] whose columns 0 and 1 are x and y (agent_attrs or viewer_attrs)"""
    assert view_codes.ndim == 5 and view_codes.shape[1:] == (4, 5, N, N) and view_codes.dtype == np.uint8
    ids = viewers_of(mask)
    rows = view_codes[:, ids]
    if not centred:
        return np.ascontiguousarray(rows)
    n, k, r, s = len(rows), len(ids), radius, 2 * radius + 1
    # the board in the middle of a sheet that reads "off the board" r cells around it: cell (x, y) lies at [y + r][x + r], so the
    # crop's corner (x_v - r, y_v - r) lies at [y_v][x_v]
    sheet = np.zeros((n, k, 5, N + 2 * r, N + 2 * r), dtype=np.uint8)
    sheet[:, :, 0] = FOG
    sheet[:, :, :, r:r + N, r:r + N] = rows
    out = np.empty((n, k, 5, s, s), dtype=np.uint8)
    for e in range(n):
        for j, v in enumerate(ids):
            x, y = int(agent_attrs[e, v, 0]), int(agent_attrs[e, v, 1])
            out[e, j] = sheet[e, j, :, y:y + s, x:x + s]
    return out


def compact_viewer_attrs(viewer_attrs: np.ndarray, mask: int) -> np.ndarray:
    """int32 [n, k, 12] of the four-view call's int32 [n, 4, 12]"""
    assert viewer_attrs.ndim == 3 and viewer_attrs.shape[1:] == (4, 12)
    return np.ascontiguousarray(viewer_attrs[:, viewers_of(mask)])
