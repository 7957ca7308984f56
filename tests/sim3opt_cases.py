"""Seeded scenes for OptimizeSim3 (reference src/cOptimizerLoopStuff.cpp:63-270) on the Lafida rig
(3 cameras): one keyframe KF1 against T candidates under a true Sim3, pixel noise scaled by the
pyramid level, in the terms of the C ABI (include/mcs_matcher.h): keyframe dicts as
mcs_amd.sim3_match, matches12 / ok / first2 per slot.

The observations follow the model AS WRITTEN: e12 of slot i projects with camera
keypoint_to_cam1[i2], e21 with keypoint_to_cam2[i].  Keypoint j of every keyframe belongs to
camera j % 3, so a pair with i2 % 3 == i % 3 has crossed == own cameras; every case also has
`cross` pairs with i2 % 3 != i % 3, which are consistent under the crossed lookup and gross
outliers under MCS_SIM3OPT_OWN_CAMERA.

  CASES            name -> parameters (the table of DESIGN 3.13)
  make_case(name)  -> dict
  write_case_file  the text form both C++ programs read (tests/cpp/sim3opt_io.hpp)
  parse_results    their output -> list of dicts per candidate
  digest(case)     SHA-256 over the inputs, stored in the fixture
"""
import hashlib

import numpy as np

C, L, W, H = 3, 8, 754, 480
OWN_CAMERA = 1


def make_rig():
    from mcs_amd import ba_synth, fuse, synth
    cams = synth.LAFIDA_CAMS[:C]
    return dict(m_c=np.stack([fuse.cayley2hom(np.array(m)) for m in synth.LAFIDA_MC[:C]]),
                cam=np.stack([ba_synth.cam_vec(c) for c in cams]), cams=cams,
                scale=1.2 ** np.arange(L), mirror=np.ones((C, 2, 2), np.uint8),
                grid_params=np.tile(np.array([0.0, 0.0, 64.0 / W, 48.0 / H]), (C, 1)))


def w2i(cam, p):
    """WorldToImg (src/cam_model_omni.cpp:147-163), cam = c d e u0 v0 invP[12]."""
    x, y, z = (float(v) for v in p)
    n = np.sqrt(x * x + y * y) or 1e-14
    th = np.arctan(-z / n)
    rho = 0.0
    for a in cam[5:17][::-1]:
        rho = rho * th + float(a)
    uu, vv = x / n * rho, y / n * rho
    return np.array([uu * cam[0] + vv * cam[1] + cam[3], uu * cam[2] + vv + cam[4]])


def cayley_rot(c):
    from mcs_amd import fuse
    return fuse.cayley2hom(np.concatenate([c, np.zeros(3)]))[:3, :3]


def _pixel(rng, cam, rmax=200.0):
    ang, rad = rng.uniform(0, 2 * np.pi), rmax * np.sqrt(rng.uniform(0.02, 1.0))
    return np.array([cam["u0"] + rad * np.cos(ang), cam["v0"] + rad * np.sin(ang)])


def _in_view(rig, c, p_rig, rmax=235.0):
    pc = np.linalg.inv(rig["m_c"][c]) @ np.append(p_rig, 1.0)
    uv = w2i(rig["cam"][c], pc[:3])
    cam = rig["cams"][c]
    return pc[2] > 0.05 and np.hypot(uv[0] - cam["u0"], uv[1] - cam["v0"]) < rmax, uv


# name -> n1, per candidate (n2, kept, gross outliers, cross pairs), the true scale, the start's
# perturbation (rotation rad, translation, log scale), flags and what else the case scripts
CASES = {
    "A_clean": dict(seed=101, n1=96, cands=[(96, 40, 0, 5)], s=1.1, start=(0.03, 0.08, 0.06)),
    "B_outliers": dict(seed=102, n1=160, cands=[(170, 130, 20, 6)], s=1.7, start=(0.02, 0.05, 0.04)),
    "C_batch": dict(seed=103, n1=96, cands=[(90, 0, 0, 0), (96, 2, 0, 0), (100, 3, 0, 1), (96, 70, 4, 4)], s=0.9,
                    start=(0.02, 0.05, 0.04)),
    "D_below3": dict(seed=104, n1=48, cands=[(48, 5, 3, 1)], s=1.2, start=(0.01, 0.02, 0.02)),
    "E_skips": dict(seed=105, n1=96, cands=[(96, 36, 3, 4)], s=0.6, start=(0.02, 0.05, 0.04), skips=True, top=True),
    "F_gainstop": dict(seed=106, n1=96, cands=[(96, 40, 0, 4)], s=1.0, start=(0.0, 0.0, 0.0)),
    "G_own_camera": dict(seed=102, n1=160, cands=[(170, 130, 20, 6)], s=1.7, start=(0.02, 0.05, 0.04),
                         flags=OWN_CAMERA),
    "H_undefined": dict(seed=108, n1=48, cands=[(96, 30, 2, 3)], s=1.3, start=(0.02, 0.05, 0.04), beyond=6),
    # in every case above the reference's gain stop fires in round 1, so its round 2 runs no
    # iteration; with optimize(2) as round 1 the flag stays down and round 2 iterates
    "I_round2": dict(seed=109, n1=96, cands=[(96, 40, 3, 4)], s=1.1, start=(0.2, 0.5, 0.3), opts=dict(its_round1=2)),
    # the kernel walks the slots, and the culled rows, in rounds of 256: the cases below are the
    # smallest that enter a second round (J: two slot rounds, rows above 256, the skip rules on
    # slots >= 256 and undefined slots on both sides of 256), a third, partial one in a batch (K:
    # more than 256 pairs, exactly 257, none, and fewer than 3 left after the cull) and a round 2
    # that iterates over more than 256 rows left by the cull (L)
    "J_rounds": dict(seed=110, n1=400, cands=[(420, 300, 12, 6)], s=1.7, start=(0.02, 0.05, 0.04), skips=True,
                     skip_from=256, beyond=6, beyond_every=50),
    "K_batch_wide": dict(seed=111, n1=520, cands=[(540, 300, 12, 6), (530, 257, 0, 4), (520, 0, 0, 0), (520, 5, 3, 1)],
                         s=0.9, start=(0.02, 0.05, 0.04)),
    "L_round2_wide": dict(seed=112, n1=400, cands=[(420, 300, 13, 6)], s=1.1, start=(0.2, 0.5, 0.3),
                          opts=dict(its_round1=2), out_every=24),
}
NOISE = 0.15     # pixel noise = NOISE * scale[octave]


def make_case(name):
    from mcs_amd import fuse, synth
    P = CASES[name]
    rng = np.random.default_rng(P["seed"])
    rig = make_rig()
    n1 = P["n1"]
    top = 8 if P.get("top") else 4
    Mt1 = fuse.cayley2hom(np.concatenate([rng.uniform(-0.03, 0.03, 3), rng.uniform(-0.05, 0.05, 3)]))
    s12 = float(P["s"])
    R12, t12 = cayley_rot(rng.uniform(-0.05, 0.05, 3)), rng.uniform(-0.2, 0.2, 3)
    n_cross = max(c[3] for c in P["cands"])
    cam_a = np.arange(n1) % C                 # keypoint_to_cam1[i2] of the slot's pairs
    cross = rng.choice(n1, n_cross, replace=False) if n_cross else np.zeros(0, int)
    cam_a[cross] = (cam_a[cross] + 1 + rng.integers(0, C - 1, len(cross))) % C
    # every slot of KF1: a point seen by camera a in KF1 and by camera i % C from the other side
    xy1, oct1, X1 = np.zeros((n1, 2), np.float32), rng.integers(0, top, n1).astype(np.int32), np.zeros((n1, 3))
    for i in range(n1):
        a, b = int(cam_a[i]), i % C
        for tries in range(400):
            px = _pixel(rng, rig["cams"][a])
            ray = np.array(synth.img_to_world(rig["cams"][a], np.array([px[0]]), np.array([px[1]]))).reshape(3)
            p = (rig["m_c"][a] @ np.append(ray * rng.uniform(0.8, 6.0), 1.0))[:3]
            if a == b or _in_view(rig, b, R12.T @ (p - t12) / s12)[0] or tries == 399:
                break
        X1[i] = p
        xy1[i] = _in_view(rig, a, p)[1] + rng.normal(0, NOISE * rig["scale"][oct1[i]], 2)
    kf1 = dict(kp_xy=xy1, kp_octave=oct1, kp_cam=(np.arange(n1) % C).astype(np.int32),
               desc=np.zeros((n1, 32), np.uint8), mask=None, m_t=Mt1)
    pts1 = dict(pos=(Mt1[:3, :3] @ X1.T).T + Mt1[:3, 3], dist=np.ones((n1, 2)), desc=np.zeros((n1, 32), np.uint8),
                mask=None)
    ok1 = np.ones(n1, np.uint8)
    T = len(P["cands"])
    case = dict(name=name, rig=rig, kf1=kf1, pts1=pts1, ok1=ok1, kf2s=[], pts2s=[], ok2s=[], first2s=[],
                matches12=np.full((T, n1), -1, np.int32), s12=np.zeros(T), R12=np.zeros((T, 9)),
                t12=np.zeros((T, 3)), flags=int(P.get("flags", 0)),
                opts=dict(default_options(), **P.get("opts", {})), inv_sigma2_1=1.0 / rig["scale"] ** 2, sigma2_2=rig["scale"] ** 2, undefined=[], truth=[])
    for t, (n2, kept, n_out, n_cr) in enumerate(P["cands"]):
        Mt2 = fuse.cayley2hom(np.concatenate([rng.uniform(-0.03, 0.03, 3), rng.uniform(-0.05, 0.05, 3)]))
        xy2 = np.stack([_pixel(rng, rig["cams"][j % C]) for j in range(n2)]).astype(np.float32)
        oct2 = rng.integers(0, top, n2).astype(np.int32)
        pos2 = rng.normal(0, 3.0, (n2, 3))
        ok2, first2 = np.ones(n2, np.uint8), np.arange(n2, dtype=np.int32)
        plain = np.setdiff1d(np.arange(min(n1, n2)), cross)
        slots = np.concatenate([rng.choice(cross, n_cr, replace=False),
                                rng.choice(plain, kept - n_cr, replace=False)]).astype(int) if kept else np.zeros(0, int)
        free = list(rng.permutation(n2))
        undefined, out_left = [], n_out
        for j, i in enumerate(sorted(slots)):
            a = int(cam_a[i])
            beyond = P.get("beyond", 0) and j % P.get("beyond_every", 5) == 2 and len(undefined) < P["beyond"]
            i2 = next(k for k in free if k % C == a and ((k >= n1) if beyond else (k < n1)))
            free.remove(i2)
            if beyond:
                undefined.append(int(i))
            m = i2
            if P.get("skips") and j % 6 == 1:            # observed first at another keypoint than its slot
                m = next(k for k in free if k != i2)
                free.remove(m)
            X2 = R12.T @ (X1[i] - t12) / s12
            uv = _in_view(rig, i % C, X2)[1] + rng.normal(0, NOISE * rig["scale"][oct2[i2]] ** -1, 2)
            every = P.get("out_every", 1)                    # gross outliers: the first plain pairs, or every n-th
            if out_left and i not in cross and not beyond and j % every == 0:
                out_left -= 1
                uv = uv + rng.choice([-1, 1], 2) * rng.uniform(30, 80, 2)
            xy2[i2] = uv
            pos2[m] = Mt2[:3, :3] @ X2 + Mt2[:3, 3]
            first2[m] = i2
            case["matches12"][t, i] = m
        if P.get("skips"):                               # one of each skip rule, on slots not kept
            spare = [i for i in range(P.get("skip_from", 0), min(n1, n2)) if i not in slots][:4]
            ms = [free.pop() for _ in spare]
            for i, m in zip(spare, ms):
                case["matches12"][t, i] = m
            ok1[spare[0]] = 0                            # NULL or bad pMP1
            ok2[ms[1]] = 0                               # bad pMP2
            first2[ms[2]] = -1                           # pMP2 does not observe KF2
            ok1[spare[3]], ok2[ms[3]] = 0, 0
        w = rng.normal(size=3)
        dR = cayley_rot(P["start"][0] * w / np.linalg.norm(w) / 2)
        case["s12"][t] = s12 * float(np.exp(P["start"][2] * rng.uniform(-1, 1)))
        case["R12"][t] = (dR @ R12).reshape(9)
        case["t12"][t] = t12 + P["start"][1] * rng.uniform(-1, 1, 3)
        case["kf2s"].append(dict(kp_xy=xy2, kp_octave=oct2, kp_cam=(np.arange(n2) % C).astype(np.int32),
                                 desc=np.zeros((n2, 32), np.uint8), mask=None, m_t=Mt2))
        case["pts2s"].append(dict(pos=pos2, dist=np.ones((n2, 2)), desc=np.zeros((n2, 32), np.uint8), mask=None))
        case["ok2s"].append(ok2)
        case["first2s"].append(first2)
        case["undefined"].append(undefined)
        case["truth"].append((s12, R12, t12))
    return case


def without_undefined(case):
    """The matches the reference run of the case gets: the slots whose crossed lookup leaves its map
    taken out (the text dereferences end() there)."""
    m = case["matches12"].copy()
    for t, u in enumerate(case["undefined"]):
        m[t, u] = -1
    return m


def default_options():
    return dict(std_sim=4.0, its_round1=5, its_clean=5, its_culled=10, terminate_max_iter=15, gain_threshold=1e-6,
                tau=1e-5, max_trials=10)


def _fmt(a):
    return " ".join("%.17g" % float(v) for v in np.asarray(a, np.float64).reshape(-1))


def _kf_lines(kf, pts):
    rows = ["%.9g %.9g %d %d" % (float(x), float(y), int(o), int(c))
            for (x, y), o, c in zip(np.asarray(kf["kp_xy"], np.float32), kf["kp_octave"], kf["kp_cam"])]
    return rows + [_fmt(kf["m_t"]), _fmt(pts["pos"])]


def write_case_file(case, path, matches12=None, flags=None):
    o = case["opts"]
    m12 = case["matches12"] if matches12 is None else matches12
    T, n1 = m12.shape
    out = ["%d %d %d %d %d" % (T, n1, C, L, case["flags"] if flags is None else flags),
           "%.17g %d %d %d %d %.17g %.17g %d" % (o["std_sim"], o["its_round1"], o["its_clean"], o["its_culled"],
                                                  o["terminate_max_iter"], o["gain_threshold"], o["tau"],
                                                  o["max_trials"])]
    out += _kf_lines(case["kf1"], case["pts1"]) + [" ".join(str(int(v)) for v in case["ok1"])]
    out += [_fmt(case["rig"]["m_c"]), _fmt(case["rig"]["cam"]), _fmt(case["inv_sigma2_1"]), _fmt(case["sigma2_2"])]
    for t in range(T):
        kf2 = case["kf2s"][t]
        out += [str(len(kf2["kp_xy"]))] + _kf_lines(kf2, case["pts2s"][t])
        out += [" ".join(str(int(v)) for v in case["ok2s"][t]), " ".join(str(int(v)) for v in case["first2s"][t]),
                " ".join(str(int(v)) for v in m12[t]), "%.17g" % case["s12"][t], _fmt(case["R12"][t]),
                _fmt(case["t12"][t])]
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def parse_results(text, n1):
    """The lines of s3io::print_out -> list of dicts, one per candidate."""
    res = []
    for line in text.splitlines():
        k, *v = line.split()
        if k == "cand":
            res.append({})
        elif k == "counts":
            res[-1].update(zip(("n_in", "n_corr", "n_bad", "n_undefined"), map(int, v)))
        elif k == "sim3":
            f = [float(x) for x in v]
            res[-1].update(s=f[0], q=np.array(f[1:5]), t=np.array(f[5:8]))
        elif k == "iters":
            res[-1]["iters"] = np.array(v, np.int32)
        elif k in ("chi2", "lambda"):
            res[-1][k] = np.array([float(x) for x in v])
        elif k in ("trials0", "trials1"):
            res[-1].setdefault("trials", np.zeros((2, 16), np.int32))[int(k[-1])] = np.array(v, np.int32)
        elif k == "matches":
            res[-1]["matches12"] = np.array(v, np.int32).reshape(n1)
        elif k in ("edge_chi2", "edge_chi2_r1"):
            res[-1][k] = np.array([float(x) for x in v]).reshape(n1, 2)
    return res


def digest(case):
    h = hashlib.sha256()
    for a in ([case["kf1"]["kp_xy"], case["kf1"]["kp_octave"], case["kf1"]["m_t"], case["pts1"]["pos"], case["ok1"],
               case["matches12"], case["s12"], case["R12"], case["t12"]] +
              [x for t in range(len(case["kf2s"]))
               for x in (case["kf2s"][t]["kp_xy"], case["kf2s"][t]["kp_octave"], case["kf2s"][t]["m_t"],
                         case["pts2s"][t]["pos"], case["ok2s"][t], case["first2s"][t])]):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# ----------------------------------------------------------------------------- the comparison
REALS = ("s", "q", "t", "chi2", "edge_chi2")
FLOOR = 1e-9          # the project's floor for edge math, relative to the field's scale


def _scale(field, want):
    if field == "q":
        return 1.0
    w = np.asarray(want, np.float64).reshape(-1)
    w = w[~np.isnan(w)]
    return float(np.abs(w).max()) if len(w) else 1.0


def tolerance(fix, name, field, t):
    """max(8 x the spread of the reference's three difference steps, 1e-9 of the field's scale)."""
    return max(8.0 * float(fix["measured_%s_%s" % (name, field)][t]),
               FLOOR * _scale(field, fix["%s_%s" % (name, field)][t]))


def compare(fix, name, got, exact=("n_in", "n_corr", "n_bad", "n_undefined", "iters", "trials", "matches12"),
            out=print):
    """A list of result dicts (one per candidate) against the fixture: integers and sets exact,
    reals to `tolerance`.  Prints every figure before it asserts."""
    T = len(fix[name + "_n_in"])
    assert len(got) == T
    for t in range(T):
        g = got[t]
        for f in exact:
            if f not in g:
                continue
            want = fix["%s_%s" % (name, f)][t]
            assert np.array_equal(np.asarray(g[f]), want), "%s[%d] %s: %s != %s" % (name, t, f, g[f], want)
        kept = ~np.isnan(fix[name + "_edge_chi2"][t])
        assert np.array_equal(~np.isnan(g["edge_chi2"]), kept), "%s[%d]: kept slots differ" % (name, t)
        for f in REALS:
            want = np.asarray(fix["%s_%s" % (name, f)][t], np.float64)
            have = np.asarray(g[f], np.float64)
            if f == "q":
                d = min(np.abs(have - want).max(), np.abs(have + want).max())
            else:
                ok = ~np.isnan(want.reshape(-1))
                d = float(np.abs(have.reshape(-1)[ok] - want.reshape(-1)[ok]).max()) if ok.any() else 0.0
            tol = tolerance(fix, name, f, t)
            out("%s[%d] %-9s diff %.3e  tol %.3e" % (name, t, f, d, tol))
            assert d <= tol, "%s[%d] %s: %.3e above %.3e" % (name, t, f, d, tol)


# ----------------------------------------------------------------------------- the C ABI's view
def call_args(case):
    """The positional arguments of mcs_amd.sim3_opt.optimize_sim3 / pack_call for a case."""
    return (case["rig"], case["kf1"], case["pts1"], case["kf2s"], case["pts2s"], case["matches12"], case["ok1"],
            case["ok2s"], case["first2s"])


def results_of(out, matches12):
    """The arrays of mcs_sim3_opt_out (NumPy, by name) -> the list of dicts `compare` takes."""
    T = len(out["n_in"])
    res = []
    for t in range(T):
        r = {k: int(out[k][t]) for k in ("n_in", "n_corr", "n_bad", "n_undefined")}
        r.update(s=float(out["s12"][t]), q=np.asarray(out["q12"][t]), t=np.asarray(out["t12"][t]),
                 iters=np.asarray(out["iters"][t]), chi2=np.asarray(out["chi2"][t]),
                 trials=np.asarray(out["trials"][t]), matches12=np.asarray(matches12[t]),
                 edge_chi2=np.asarray(out["edge_chi2"][t]), R=np.asarray(out["R12"][t]),
                 lam=np.asarray(out["lambda"][t]))
        res.append(r)
    return res
