#!/usr/bin/env python3
"""Generate tests/golden/analysis.npz by RUNNING THE REFERENCE'S OWN STATEMENTS of its analysis layer.

Run only in the build container (needs /root/reference; the GPU box never sees it):
    python tests/golden/make_analysis_golden.py

In the manner of make_golden.py: the reference files are parsed, the statements that compute numbers are pulled out by AST,
compiled on their own and executed with this container's pandas / NumPy; nothing that plots, prints a path or writes a file is
run, and no reference source text is stored - the .npz holds the inputs and the numbers those statements returned.
  3d_reconstruction.py  MarkerAnalysis.analyze_displacement: the assignments of :332-334 (sort, cumulative sum) and :397-400
                        (the statistics table)
  LocalAnalysis.py      calculate_average_coordinates (:53-60) as a whole; of analyze_displacement the assignments :81-93
                        (inner merge, dX / dY / dZ, norms)
  MarkerDisplacement.py plot_marker_displacement: the SCALAR branch's statements :161-173 (start position, distance)

The case: a float32 table [160, 19, 10] and disp [160, 19, 5] on the ids (0,0), (1,0..5), (2,0..11), built below and STORED in
the file (tests read them from there, never from the seed).  It holds: a slot never seen (3); a slot with exactly one
displacement row (5, seen in frames 10 and 11 only); a slot absent from the second window (9); a slot whose mean displacement
is more than 100 times its standard deviation (11: the cancellation case); gaps inside both windows (2, 4 and the random 3 %);
frame 0 present for most slots, absent for 3, 5 and 7.
"""
import ast
import os
import sys

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference/code"
R3 = os.path.join(REF, "Marker_Calibration", "3d_reconstruction.py")
LA = os.path.join(REF, "ForceDistribution", "LocalAnalysis.py")
MDP = os.path.join(REF, "ForceDistribution", "MarkerDisplacement.py")

N, START, END = 160, (1, 30), (120, 150)


def _function(path, name, cls=None):
    src = open(path).read()
    body = ast.parse(src).body
    if cls is not None:
        body = next(n for n in body if isinstance(n, ast.ClassDef) and n.name == cls).body
    return next(n for n in body if isinstance(n, ast.FunctionDef) and n.name == name)


def _target_names(st):
    names = set()
    for t in st.targets:
        for node in ast.walk(t):
            if isinstance(node, ast.Name):
                names.add(node.id)
    return names


def _compile(name, args, statements, ret, env):
    """def name(args): <statements>; return ret"""
    fn = ast.parse(f"def {name}({args}):\n    pass").body[0]
    fn.body = list(statements) + [ast.parse(f"return {ret}").body[0]]
    mod = ast.Module(body=[fn], type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = dict(env)
    exec(compile(mod, f"<{name} from reference>", "exec"), ns)
    return ns[name]


def assignments(statements, lo, hi, names):
    """The assignment statements within source lines [lo, hi] whose targets are among `names`."""
    return [st for st in statements if isinstance(st, ast.Assign) and lo <= st.lineno and st.end_lineno <= hi
            and _target_names(st) <= set(names)]


def reference_functions():
    env = dict(np=np, pd=pd)
    ad = _function(R3, "analyze_displacement", "MarkerAnalysis")
    keep = assignments(ad.body, 332, 334, {"results_df"}) + assignments(ad.body, 397, 400, {"stats"})
    assert len(keep) == 3, len(keep)
    stats_fn = _compile("stats_fn", "results_df", keep, "(results_df, stats)", env)

    avg = _function(LA, "calculate_average_coordinates")
    mod = ast.Module(body=[avg], type_ignores=[])
    ns = dict(env)
    exec(compile(mod, "<calculate_average_coordinates from reference>", "exec"), ns)
    avg_fn = ns["calculate_average_coordinates"]
    la = _function(LA, "analyze_displacement")
    tr = next(n for n in la.body if isinstance(n, ast.Try))
    keep = assignments(tr.body, 81, 93, {"merged", "magnitudes"})
    assert len(keep) == 5, len(keep)
    merge_fn = _compile("merge_fn", "start_avg, end_avg", keep, "(merged, magnitudes)", env)

    pm = _function(MDP, "plot_marker_displacement")
    tr = next(n for n in pm.body if isinstance(n, ast.Try))
    branch = None
    for node in ast.walk(tr):
        if isinstance(node, ast.If) and isinstance(node.test, ast.Compare) and getattr(node.test.left, "id", "") == "mode" \
                and getattr(node.test.comparators[0], "value", None) == "SCALAR":
            branch = node
    keep = [st for st in branch.body if 161 <= st.lineno and st.end_lineno <= 173 and isinstance(st, (ast.Assign, ast.If))]
    assert len(keep) == 4, len(keep)                # start_pos, `if start_pos.empty: ... return`, X0 Y0 Z0, displacement
    scalar_fn = _compile("scalar_fn", "marker_data", keep, "displacement", dict(env, print=lambda *a, **k: None))
    return stats_fn, avg_fn, merge_fn, scalar_fn


def build_case():
    rng = np.random.default_rng(20240607)
    ids = np.array([(0, 0)] + [(1, i) for i in range(6)] + [(2, i) for i in range(12)], dtype=np.int64)
    m = len(ids)
    seen = rng.random((N, m)) >= 0.03
    seen[:, 3] = False                                           # never seen
    seen[:, 5] = False
    seen[[10, 11], 5] = True                                      # exactly one displacement row
    seen[0, 7] = False                                           # frame 0 absent
    seen[0, [0, 1, 2, 4, 6, 8, 9, 10, 11, 12]] = True
    seen[120:, 9] = False                                        # absent from the second window
    seen[[5, 17, 130, 141], 2] = False                           # gaps inside both windows
    seen[[9, 10, 125, 126, 127], 4] = False
    seen[1:, 11] = True
    f = np.arange(N, dtype=np.float64)[:, None]
    ang = 2 * np.pi * np.arange(m)[None, :] / m
    xyz = np.stack([18.0 * np.cos(ang) + 0.011 * f * np.cos(ang) + rng.normal(0, 0.02, (N, m)),
                    18.0 * np.sin(ang) + 0.007 * f * np.sin(ang) + rng.normal(0, 0.02, (N, m)),
                    3.0 - 0.004 * f * (1 + 0.1 * np.arange(m)[None, :]) + rng.normal(0, 0.03, (N, m))], axis=2)
    xyz[:, 11, 0] = 2.0 + 0.5 * f[:, 0] + rng.normal(0, 5e-4, N)    # a steady 0.5 per frame: mean |d| >> std
    xyz[:, 11, 1] = -4.0 + rng.normal(0, 5e-4, N)
    xyz[:, 11, 2] = 2.5 + rng.normal(0, 5e-4, N)
    xyz = np.round(xyz * 4096.0) / 4096.0                        # (a 1/4096 mm grid: the file compresses, the sums still round)
    table = np.zeros((N, m, 10), dtype=np.float32)
    table[..., 0] = np.where(seen, 3.0, 0.0)
    table[..., 1] = np.where(seen, np.round(320 + 162 * np.cos(ang)), 0)
    table[..., 2] = np.where(seen, np.round(240 + 162 * np.sin(ang)), 0)
    table[..., 3] = np.where(seen, 19.0, 0)
    table[..., 4] = np.where(seen, 18.5, 0)
    table[..., 5] = np.where(seen, 90.0, 0)
    table[..., 6:9] = np.where(seen[..., None], xyz, 0)
    # last-seen displacement of those float32 rows (3d_reconstruction.py:263-314), float64 then stored as float32
    disp = np.zeros((N, m, 5), dtype=np.float32)
    t64 = table.astype(np.float64)
    for s in range(m):
        last = None
        for fr in range(N):
            if seen[fr, s]:
                if last is not None:
                    d = t64[fr, s, 6:9] - t64[last, s, 6:9]
                    disp[fr, s] = [1.0, d[0], d[1], d[2], np.sqrt((d * d).sum())]
                last = fr
    return ids, table, disp


def main():
    from vbs_amd.ids import marker_ids
    stats_fn, avg_fn, merge_fn, scalar_fn = reference_functions()
    ids, table, disp = build_case()
    n, m = table.shape[:2]
    mid = marker_ids(ids)
    out = dict(ids=ids, table=table, disp=disp, windows=np.array([START, END], dtype=np.int64), marker_id=mid)

    # ---- analyze_displacement -------------------------------------------------------------------------------------
    d64 = disp.astype(np.float64)
    f, s = np.nonzero(d64[..., 0] != 0)
    perm = np.random.default_rng(1).permutation(len(f))            # (the reference sorts; give it something to sort)
    f, s = f[perm], s[perm]
    df = pd.DataFrame({"frameno": f, "row": ids[s, 0], "col": ids[s, 1], "displacement": d64[f, s, 4]})
    res, stats = stats_fn(df)
    counts = res.groupby(["row", "col"]).size()
    exp = np.full((m, 5), np.nan)
    exp[:, 0] = 0
    slot_of = {tuple(k): i for i, k in enumerate(ids.tolist())}
    for key, r in stats.iterrows():
        exp[slot_of[key]] = [counts[key], r[("displacement", "mean")], r[("displacement", "std")], r[("displacement", "max")],
                             r[("cumulative_displacement", "last")]]
    cum = np.full((n, m), np.nan)
    cum[res["frameno"].to_numpy(), [slot_of[k] for k in zip(res["row"], res["col"])]] = res["cumulative_displacement"].to_numpy()
    out.update(stats=exp, cumulative=cum)
    assert exp[3, 0] == 0 and exp[5, 0] == 1 and np.isnan(exp[5, 2]) and exp[11, 1] >= 100 * exp[11, 2]

    # ---- LocalAnalysis --------------------------------------------------------------------------------------------
    t64 = table.astype(np.float64)
    f, s = np.nonzero((t64[..., 0].astype(np.int64) & 2) != 0)
    sheet = pd.DataFrame({"frameno": f, "marker_id": mid[s], "Xw": t64[f, s, 6], "Yw": t64[f, s, 7], "Zw": t64[f, s, 8]})
    slot_of_id = {int(v): i for i, v in enumerate(mid)}
    target = [int(mid[i]) for i in (1, 2, 3, 4, 9, 11, 13)]
    for tag, frame in (("all", sheet), ("sel", sheet[sheet["marker_id"].isin(target)])):
        a0, a1 = avg_fn(frame, START, "start"), avg_fn(frame, END, "end")
        merged, mags = merge_fn(a0, a1)
        for w, a in enumerate((a0, a1)):
            wm = np.full((m, 3), np.nan)
            wm[[slot_of_id[int(v)] for v in a["marker_id"]]] = a.iloc[:, 1:4].to_numpy()
            out[f"win_{tag}_{w}"] = wm
        out[f"merged_{tag}_slots"] = np.array([slot_of_id[int(v)] for v in merged["marker_id"]], dtype=np.int64)
        out[f"merged_{tag}_d"] = np.concatenate([merged[["dX", "dY", "dZ"]].to_numpy(), np.asarray(mags)[:, None]], axis=1)
        out[f"merged_{tag}_mean"] = np.array(np.mean(mags))
    out["target_slots"] = np.array([slot_of_id[v] for v in target], dtype=np.int64)
    assert 9 not in out["merged_all_slots"] and 3 not in out["merged_all_slots"] and 2 in out["merged_all_slots"]

    # ---- MarkerDisplacement, SCALAR mode --------------------------------------------------------------------------
    scal = np.full((n, m), np.nan)
    for slot in range(m):
        md = sheet[sheet["marker_id"] == mid[slot]].sort_values(by="frameno").reset_index(drop=True)      # (:135)
        if md.empty:
            continue
        got = scalar_fn(md)
        if got is None:                                  # "Frame 0 data missing"
            continue
        scal[md["frameno"].to_numpy(), slot] = np.asarray(got)
    out["scalar"] = scal
    assert np.isnan(scal[:, [3, 5, 7]]).all() and np.isfinite(scal[0, 0])
    np.savez_compressed(os.path.join(HERE, "analysis.npz"), **out)
    print("analysis.npz written:", os.path.getsize(os.path.join(HERE, "analysis.npz")), "bytes; pandas", pd.__version__,
          "numpy", np.__version__)


if __name__ == "__main__":
    main()
