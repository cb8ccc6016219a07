"""Caps and recordings the tests of `vbs_sphere_series` share (`tests/test_sphere_host.py`, `tests/test_gpu_sphere.py`): seeded and
small.  A cap is a layout put onto a sphere below its centre; a press cuts it by a plane: every point beyond the plane is moved
along the plane's normal onto it.  A recording is a float32 table whose X, Y, Z columns carry such caps (`rigid_cases.table_of_points`:
every cell the contract says is not read holds NaN or a huge value).  The case makers ASSERT, on the CPU, that every decision of
every case has a relative margin (`sphere_oracle.assert_margins`) and draw the case again otherwise."""
import numpy as np

import rigid_cases as RC
import sphere_oracle as O

R0 = 27.0
C0 = np.array([0.0, 0.0, 27.0])


def cap(xy, centre=C0, radius=R0):
    """[m, 3]: the points of the sphere (centre, radius) below its centre whose x, y are `xy` + the centre's."""
    xy = np.asarray(xy, dtype=np.float64)
    z = centre[2] - np.sqrt(radius * radius - (xy ** 2).sum(axis=1))
    return np.column_stack([xy + np.asarray(centre)[:2], z])


def cap65(centre=C0, radius=R0):
    """The published 65-marker layout on an exact sphere of radius 27."""
    return cap(RC.layout65()[:, :2], np.asarray(centre, dtype=np.float64), radius)


def normal_of(tilt_deg, azimuth_deg):
    t, a = np.deg2rad(tilt_deg), np.deg2rad(azimuth_deg)
    return np.array([np.sin(t) * np.cos(a), np.sin(t) * np.sin(a), np.cos(t)])


def press(P, delta, tilt_deg=0.0, azimuth_deg=0.0, centre=C0, radius=R0):
    """The cap P cut by the plane n . (C - X) = R - delta, n leaning by `tilt_deg` towards `azimuth_deg`: the points beyond it are
    moved along n onto it.  -> (points, pressed [m]: how far each was moved, 0 for the others)."""
    n = normal_of(tilt_deg, azimuth_deg)
    over = np.maximum((np.asarray(centre) - P) @ n - (radius - delta), 0.0)
    return P + over[:, None] * n, over


def true_depth(P, centre=C0, radius=R0):
    return radius - np.sqrt(((P - np.asarray(centre)) ** 2).sum(axis=1))


def press_recording(n, still=0, delta_end=2.8, tilt_end=15.0, azimuth=35.0, noise=0.02, gaps=0.03, seed=0, centre=C0):
    """`still` unloaded frames, then n frames of the 65-marker cap cut at delta = 0 -> `delta_end` mm while leaning 0 -> `tilt_end`
    degrees towards `azimuth`, with `noise` mm on every coordinate and a share `gaps` of the rows missing (none in frame 0).
    -> dict(table, P (noise-free, float64), delta, tilt [still + n], azimuth, noise, dead)."""
    rng = np.random.default_rng(8000 + seed)
    lay = cap65(centre)
    delta = np.concatenate([np.zeros(still), np.linspace(0.0, delta_end, n)])
    tilt = np.concatenate([np.zeros(still), np.linspace(0.0, tilt_end, n)])
    clean = np.stack([press(lay, d, t, azimuth, centre)[0] for d, t in zip(delta, tilt)])
    dead = rng.random((still + n, 65)) < gaps
    dead[0] = False
    P = clean + rng.normal(size=clean.shape) * noise
    return dict(table=RC.table_of_points(P, dead, seed), P=clean, delta=delta, tilt=tilt, azimuth=azimuth, noise=noise, dead=dead,
                layout=lay)


def recording(n, m, seed=0, drop=0.1, outliers=0, empty_frame=None, bad_src=0.05, centre=(1.5, -2.0, 27.25), delta_end=2.0):
    """-> dict(table, source, layout): a jittered grid of m slots on the sphere of radius 27 about `centre`; frame f is the cap cut
    at delta = delta_end f / (n - 1) leaning 2 f degrees towards 35, with noise of 0.01 mm.  A share `drop` of the rows has no 3-D
    point, a share `bad_src` of the slots has source flag 0, `outliers` slots of every ODD frame are moved OUTWARDS by 1.5 mm (what
    the rejection of the per-frame fit removes; the even frames it leaves alone), `empty_frame` loses every row."""
    rng = np.random.default_rng(7000 + seed)
    c = np.asarray(centre, dtype=np.float64)
    side = int(np.ceil(np.sqrt(m)))
    lay = cap(RC.flat_grid(m, min(2.0, 30.0 / side), seed)[:, :2], c)
    P = np.empty((n, m, 3))
    for f in range(n):
        P[f] = press(lay, delta_end * f / max(n - 1, 1), 2.0 * f, 35.0, c)[0] + rng.normal(size=(m, 3)) * 0.01
        if outliers and f % 2 == 1:
            far = np.argsort(-((lay[:, :2] - c[:2]) ** 2).sum(axis=1))[:4 * outliers]     # (on the rim: never a contact slot)
            k = rng.choice(far, size=min(outliers, m), replace=False)
            P[f, k] += 1.5 * (P[f, k] - c) / R0
    dead = rng.random((n, m)) < drop
    if empty_frame is not None:
        dead[empty_frame] = True
    bad = rng.random(m) < bad_src
    return dict(table=RC.table_of_points(P, dead, seed), source=RC.source_of(lay, bad), layout=lay, centre=c)


def with_margins(make, run, tries=20):
    """The first of `make(seed)`, seed = 0, 1, .., every decision of which has a margin: -> (case, what `run(case)` returned).
    `run(case, margins)` computes the restatement and appends its decisions to `margins`."""
    for seed in range(tries):
        case, margins = make(seed), []
        want = run(case, margins)
        if all(v > O.MIN_MARGIN for _, v in margins):
            return case, want
    raise AssertionError("no seed gives a case whose decisions all have a margin")


def special_contacts():
    """Seven frames of the exact 65-marker cap (no noise) against the GIVEN sphere (0, 0, 27, 27) with contact sets of 0, 1, 2, 3
    (not collinear), 3 collinear, 3 coincident and many slots: chosen slots are moved to stated points inside the sphere.
    -> (table, expected n_contact [7], expected flag [7])."""
    lay = cap65()
    P = np.stack([lay] * 7)
    inside = lambda x, y: (x, y, 0.75)                            # noqa: E731  (|P - C| <= sqrt(18 + 26.25^2) = 26.59 < 26.9)
    P[1, 0] = inside(0.0, 0.0)
    P[2, 0], P[2, 1] = inside(0.0, 0.0), inside(3.0, 0.0)
    P[3, 0], P[3, 1], P[3, 2] = inside(0.0, 0.0), inside(3.0, 0.0), inside(0.0, 3.0)
    P[4, 0], P[4, 1], P[4, 2] = inside(-3.0, 0.0), inside(0.0, 0.0), inside(3.0, 0.0)
    P[5, 0] = P[5, 1] = P[5, 2] = inside(1.0, -1.0)
    P[6] = press(lay, 2.0, 6.0, 35.0)[0]
    many = float((true_depth(P[6]) > 0.1).sum())
    return RC.table_of_points(P), np.array([0.0, 1.0, 2.0, 3.0, 3.0, 3.0, many]), np.array([1.0, 2.0, 2.0, 3.0, 2.0, 2.0, 3.0])
