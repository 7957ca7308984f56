"""Seeded cases of cOptimizer::OptimizeEssentialGraph (reference src/cOptimizerLoopStuff.cpp:273-519)
for tests/golden/gen_essgraph_ref.py and the essgraph tests: a drifted keyframe chain that a loop
closes, as flat arrays (keyframes in ascending id order), the text file both C++ programs read
(tests/cpp/essgraph_io.hpp), the parser of their result lines and the parity rule.

A Sim3 is 8 doubles: s, qw qx qy qz, tx ty tz.  Non-corrected Sim3s are the drifted SE3 poses
(scale 1); the current keyframe and `n_corr - 1` neighbours carry a corrected Sim3
S_i,nc * S_cur,nc^-1 * S_cur,corrected, which is how CorrectLoop propagates it.
"""
import hashlib

import numpy as np

FLOOR = 1e-9
REALS = ("sim3", "pose", "points", "chi2", "edge_chi2")
INTS = ("edges", "counts", "iterations", "trials")

ONE_TRIAL = dict(iterations=1, max_trials=1, lambda0=1e-2)

# drift = (rotation rad, translation, scale) accumulated over the whole chain
CASES = {
    "A_ring6": dict(seed=111, N=6, drift=(0.05, 0.15, 1.05), P=12),
    "B_ring12": dict(seed=112, N=12, drift=(0.08, 0.3, 1.08), P=12),
    "C_cov40": dict(seed=313, N=40, drift=(0.10, 0.5, 1.10), P=200, cov=True, n_corr=4),
    "D_gaps": dict(seed=114, N=15, drift=(0.06, 0.2, 1.06), P=12, gaps=True, loop=7),
    "E_consistent": dict(seed=15, N=10, drift=None, P=12),
    "F_large": dict(seed=16, N=12, drift=(0.3, 0.4, 1.3), P=12),
    # One trial at a moderate first damping: one linearisation, assembly, solve, update and chi2 at
    # sizes past one round of every kernel (a full run is not reproducible there).
    # G: the loop keyframe in a middle tile, 11 tiles of band 2, three chi2 partials; H: the content
    # of C_cov40 at 15 tiles with a wide band; J: more than 256 keyframes and points, 33 tiles;
    # I: more than 16384 edges (the stride loop of k_chi2, all 64 partials), band 8 of 33 tiles.
    # One damped step reaches the keyframes next to the fixed one, and those before it, only
    # through neighbours several keyframes apart: with nbr below 6 (G) and 30 (J) fewer than 90 %
    # of the keyframes move by 100 tolerances, which the generator demands
    "G_mid100": dict(seed=201, N=100, drift=(0.10, 0.5, 1.10), P=12, nbr=6, loop=37, opts=ONE_TRIAL),
    "H_cov130": dict(seed=224, N=130, drift=(0.10, 0.5, 1.10), P=200, cov=True, n_corr=4, nbr=4, opts=ONE_TRIAL),
    "J_n300": dict(seed=252, N=300, drift=(0.10, 0.5, 1.10), P=600, nbr=30, opts=ONE_TRIAL),
    "I_dense300": dict(seed=242, N=300, drift=(0.05, 0.25, 1.05), P=12, nbr=62, opts=ONE_TRIAL),
}


# ---------------------------------------------------------------------------- Sim3 in NumPy
def qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
                     a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]])


def qrot(q, v):
    w, u = q[0], q[1:]
    uv = 2.0 * np.cross(u, v)
    return v + w * uv + np.cross(u, uv)


def qaxis(rotvec):
    th = np.linalg.norm(rotvec)
    if th == 0.0:
        return np.array([1.0, 0.0, 0.0, 0.0])
    return np.concatenate([[np.cos(th / 2)], np.sin(th / 2) * np.asarray(rotvec) / th])


def smul(a, b):
    return np.concatenate([[a[0] * b[0]], qmul(a[1:5], b[1:5]), a[0] * qrot(a[1:5], b[5:8]) + a[5:8]])


def sinv(a):
    qc = a[1:5] * np.array([1.0, -1.0, -1.0, -1.0])
    return np.concatenate([[1.0 / a[0]], qc, qrot(qc, (-1.0 / a[0]) * a[5:8])])


def smap(a, x):
    return a[0] * qrot(a[1:5], x) + a[5:8]


def sim3(s, rotvec, t):
    return np.concatenate([[s], qaxis(rotvec), np.asarray(t, np.float64)])


# ---------------------------------------------------------------------------- the cases
def _csr(rows):
    ptr = np.zeros(len(rows) + 1, np.int32)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    flat = [x for r in rows for x in r]
    return ptr, flat


def make_case(name, seed=None):
    P = CASES[name]
    rng = np.random.default_rng(P["seed"] if seed is None else seed)
    N = P["N"]
    loop = P.get("loop", 0)
    cur = N - 1
    ids = np.arange(N, dtype=np.int64) + 3
    if P.get("gaps"):
        ids = np.sort(rng.choice(np.arange(2, 60), N, replace=False)).astype(np.int64)
    # truth: camera centres on a circle that closes between cur and loop; Siw maps world -> keyframe
    Snc = np.zeros((N, 8))
    span = max(1, cur - loop)
    axis, tdir = rng.normal(size=3), rng.normal(size=3)      # the seed sets the drift's directions and size
    axis, tdir = axis / np.linalg.norm(axis), tdir / np.linalg.norm(tdir)
    jit = rng.uniform(0.9, 1.1, 2)
    for i in range(N):
        f = (i - loop) / span                                  # 0 at the loop keyframe, 1 at the current
        if P["drift"] is None:                                 # exact arithmetic: identity rotations, integers
            Snc[i] = sim3(1.0, np.zeros(3), [float(i - loop), float((i * 3) % 5), -2.0 * (i - loop)])
            continue
        ang = 2 * np.pi * (i - loop) / (span + 1)
        centre = 4.0 * np.array([np.cos(ang), np.sin(ang), 0.05 * i])
        rv = np.array([0.02 * i, -0.03 * i, ang])
        rot, tr, sc = P["drift"]
        rot, tr = rot * jit[0], tr * jit[1]
        drift = sim3(1.0, rot * f * axis, tr * f * tdir)
        true = sim3(1.0, rv, [0, 0, 0])
        true[5:8] = -qrot(true[1:5], centre * (1.0 + (sc - 1.0) * f))   # scale drift stretches the track
        Snc[i] = smul(drift, true)
        Snc[i][0] = 1.0
    Scw = Snc.copy()
    has_corr = np.zeros(N, np.uint8)
    n_corr = P.get("n_corr", 1) if P["drift"] is not None else 0
    if n_corr:
        rot, tr, sc = P["drift"]
        gamma = sinv(sim3(sc, rot * jit[0] * axis, tr * jit[1] * tdir))       # what the loop found
        cur_corr = smul(gamma, Snc[cur])
        for i in range(cur - n_corr + 1, cur + 1):
            Scw[i] = smul(smul(Snc[i], sinv(Snc[cur])), cur_corr)
            has_corr[i] = 1
    parent = np.arange(-1, N - 1, dtype=np.int32)
    loops = [[] for _ in range(N)]
    cov = [[] for _ in range(N)]
    lc = [[] for _ in range(N)]
    for i in range(1, N):
        cov[i].append((i - 1, 150))
        cov[i - 1].append((i, 150))
    for k in range(2, P.get("nbr", 1) + 1):                    # a denser covisibility graph (tools/essential_graph_bench.py)
        for i in range(k, N):
            cov[i].append((i - k, 150))
            cov[i - k].append((i, 150))
    lc[cur].append((loop, 30))                                 # (current, loop) is kept below the weight
    if P.get("cov"):
        for i in range(2, N):                                  # second neighbours at 99 / 100 / 101
            w = 99 + i % 3
            cov[i].append((i - 2, w))
            cov[i - 2].append((i, w))
        loops[20].append(5)                                    # an earlier loop: only 5 < 20 adds it
        loops[5].append(20)
        lc[cur] = [(0, 30), (1, 120), (2, 80)]                 # kept (exempt), kept, dropped
        lc[cur - 1] = [(0, 100), (1, 99)]                      # kept, dropped
        lc[cur - 2] = [(0, 99), (2, 101)]                      # dropped (not the current), kept
        cov[cur].append((1, 120))                              # the fused pair is covisible too: two edges
        cov[1].append((cur, 120))
    lp, li = _csr(loops)
    cp, cf = _csr(cov)
    lcp, lcf = _csr(lc)
    npts = P["P"]
    ref = rng.integers(0, N, npts)
    pos = np.zeros((npts, 3))
    for j in range(npts):
        pos[j] = smap(sinv(Scw[ref[j]]), rng.uniform(-1, 1, 3) + np.array([0, 0, 3.0]))
        if P["drift"] is None:
            pos[j] = np.round(pos[j])
    corrected_by = np.full(npts, -1, np.int64)
    corrected_ref = np.full(npts, -1, np.int64)
    bad = (rng.uniform(size=npts) < 0.1).astype(np.uint8)
    for j in range(0, npts, 3):                                # every third point was moved by the current keyframe
        corrected_by[j] = ids[cur]
        corrected_ref[j] = ids[cur - (j // 3) % max(1, n_corr)]
    return dict(name=name, N=N, P=npts, cur=cur, loop=loop, min_weight=100, ids=ids, parent=parent,
                has_corr=has_corr, Scw=Scw, Snc=Snc, loop_ptr=lp, loop_idx=np.array(li, np.int32),
                cov_ptr=cp, cov_idx=np.array([c for c, _ in cf], np.int32), cov_w=np.array([w for _, w in cf], np.int32),
                lc_ptr=lcp, lc_idx=np.array([c for c, _ in lcf], np.int32), lc_w=np.array([w for _, w in lcf], np.int32),
                pos=pos, corrected_by=corrected_by, corrected_ref=corrected_ref, ref_kf=ids[ref], bad=bad,
                opts=dict(default_options(), **P.get("opts", {})))


def default_options():
    return dict(iterations=20, terminate_max_iter=15, gain_threshold=1e-6, lambda0=1e-6, max_trials=10)


def point_refs(case):
    """:501-507 on the host -> keyframe index per point."""
    idx = {int(v): i for i, v in enumerate(case["ids"])}
    cur_id = int(case["ids"][case["cur"]])
    return np.array([idx[int(r if b == cur_id else k)] for b, r, k in
                     zip(case["corrected_by"], case["corrected_ref"], case["ref_kf"])], np.int32)


def _fmt(a):
    return " ".join("%.17g" % float(v) for v in np.asarray(a, np.float64).reshape(-1))


def write_case_file(case, path):
    o = case["opts"]
    N = case["N"]
    rows = ["%d %d %d %d %d %d %d %d %.17g %.17g" % (N, case["P"], case["cur"], case["loop"], case["min_weight"],
                                                     o["iterations"], o["terminate_max_iter"], o["max_trials"],
                                                     o["gain_threshold"], o["lambda0"])]
    for i in range(N):
        rows.append("%d %d %d %s %s" % (case["ids"][i], case["parent"][i], case["has_corr"][i], _fmt(case["Scw"][i]),
                                        _fmt(case["Snc"][i])))
    for ptr, idx, w in ((case["loop_ptr"], case["loop_idx"], None), (case["cov_ptr"], case["cov_idx"], case["cov_w"]),
                        (case["lc_ptr"], case["lc_idx"], case["lc_w"])):
        for i in range(N):
            a, b = ptr[i], ptr[i + 1]
            vals = [str(b - a)]
            for k in range(a, b):
                vals.append(str(int(idx[k])))
                if w is not None:
                    vals.append(str(int(w[k])))
            rows.append(" ".join(vals))
    for j in range(case["P"]):
        rows.append("%s %d %d %d %d" % (_fmt(case["pos"][j]), case["corrected_by"][j], case["corrected_ref"][j],
                                        case["ref_kf"][j], case["bad"][j]))
    with open(path, "w") as f:
        f.write("\n".join(rows) + "\n")


def parse_results(text):
    """The lines of egio::print_out / print_edges -> dict."""
    r = {}
    for line in text.splitlines():
        p = line.split()
        if not p:
            continue
        k, v = p[0], p[1:]
        if k in ("counts", "edges", "trials"):
            r[k] = np.array([int(x) for x in v], np.int32)
        elif k == "iterations":
            r[k] = int(v[0])
        elif k in ("chi2_initial", "lambda", "branch_margin"):
            r[k] = float(v[0])
        else:
            r[k] = np.array([float(x) for x in v])
    r["edges"] = r["edges"].reshape(-1, 3)
    if "sim3" in r:
        r["sim3"] = r["sim3"].reshape(-1, 8)
        r["pose"] = r["pose"].reshape(-1, 16)
        r["points"] = r["points"].reshape(-1, 3)
    return r


def digest(case):
    h = hashlib.sha256()
    for k in ("ids", "parent", "has_corr", "Scw", "Snc", "loop_ptr", "loop_idx", "cov_ptr", "cov_idx", "cov_w", "lc_ptr",
              "lc_idx", "lc_w", "pos", "corrected_by", "corrected_ref", "ref_kf", "bad"):
        h.update(np.ascontiguousarray(case[k]).tobytes())
    return h.hexdigest()


def sim3_diff(a, b):
    """Largest difference of [N][8] Sim3s; q and -q are the same rotation."""
    a, b = np.asarray(a).reshape(-1, 8), np.asarray(b).reshape(-1, 8)
    dq = np.minimum(np.abs(a[:, 1:5] - b[:, 1:5]).max(1), np.abs(a[:, 1:5] + b[:, 1:5]).max(1))
    rest = np.abs(np.delete(a, [1, 2, 3, 4], 1) - np.delete(b, [1, 2, 3, 4], 1)).max(1)
    return float(max(dq.max(), rest.max())) if len(a) else 0.0


def diff(field, a, b):
    if field == "sim3":
        return sim3_diff(a, b)
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.abs(a - b).max()) if len(a) else 0.0


def tolerance(fix, name, field):
    """max(8 x the spread of the reference's three difference steps, 1e-9 of the field's scale)
    (DESIGN 3.13's rule)."""
    want = np.asarray(fix["%s_%s" % (name, field)], np.float64).reshape(-1)
    scale = float(np.abs(want).max()) if len(want) else 0.0
    return max(8.0 * float(fix["measured_%s_%s" % (name, field)]), FLOOR * max(scale, 1e-300))


def compare(fix, name, got, out=print):
    """A result dict against the fixture: integers exact, reals to `tolerance`.  Prints every figure
    before it asserts; returns the worst difference / tolerance."""
    n_it = int(fix[name + "_iterations"])
    assert int(got["iterations"]) == n_it, (name, "iterations", got["iterations"], n_it)
    assert np.array_equal(np.asarray(got["trials"])[:n_it], fix[name + "_trials"]), (name, "trials", got["trials"])
    worst = 0.0
    fails = []
    for f in REALS:
        want = fix["%s_%s" % (name, f)]
        have = np.asarray(got[f], np.float64)
        if f == "chi2":
            have = have[:n_it]
        d, tol = diff(f, have, want), tolerance(fix, name, f)
        out("%s %-9s diff %.3e  tol %.3e  ratio %.3f" % (name, f, d, tol, d / tol))
        worst = max(worst, d / tol)
        if not d <= tol:
            fails.append((f, d, tol))
    assert not fails, (name, fails)
    return worst


# ---------------------------------------------------------------------------- log / exp list
def log_exp_inputs():
    """Inputs on both sides of the four thresholds: (`log` rows [s q t], `exp` rows [7])."""
    rng = np.random.default_rng(77)
    logs, exps = [], []
    thetas = [0.0, 1e-3, 4.4e-3, 4.5e-3, 0.5, 2.5]            # 1 - d = 1e-5 at theta = 4.472e-3
    sigmas = [0.0, 5e-6, 9.9e-6, -9.9e-6, 1.01e-5, -1.01e-5, 2e-5, 1e-3, 0.3, -0.3]
    for th in thetas:
        for sg in sigmas:
            ax = rng.normal(size=3)
            ax /= np.linalg.norm(ax)
            logs.append(sim3(np.exp(sg), th * ax, rng.uniform(-2, 2, 3)))
    for th in [0.0, 5e-6, 9.9e-6, 1.01e-5, 1e-3, 0.5, 2.5]:
        for sg in sigmas:
            ax = rng.normal(size=3)
            ax /= np.linalg.norm(ax)
            exps.append(np.concatenate([th * ax, rng.uniform(-2, 2, 3), [sg]]))
    return np.array(logs), np.array(exps)


def write_list_file(path, logs, exps):
    with open(path, "w") as f:
        for r in logs:
            f.write("log " + _fmt(r) + "\n")
        for r in exps:
            f.write("exp " + _fmt(r) + "\n")


def parse_list(text):
    logs = [[float(x) for x in ln.split()[1:]] for ln in text.splitlines() if ln.startswith("log")]
    exps = [[float(x) for x in ln.split()[1:]] for ln in text.splitlines() if ln.startswith("exp")]
    return np.array(logs).reshape(-1, 7), np.array(exps).reshape(-1, 8)
