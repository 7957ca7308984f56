"""cSim3Solver (reference src/cSim3Solver.cpp), the parts that need no GPU:

  np_draw_samples     :202-222 on a Python list that keeps its popped elements, as an unchecked
                      std::vector does; mcs_sim3_draw_samples must equal it;
  np_prepare          the constructor (:44-137) for one candidate, in the text's operation order;
  np_max_its          SetRansacParameters (:139-165) -> (mRansacMaxIts, the value before ceil);
  np_horn             computeT (:286-371) with numpy.linalg.eigh, or with a plain cyclic Jacobi;
                      the two differ by rounding only, which sets the stage-A tolerance;
  np_check            CheckInliers (:374-415) from a given (s, R, t): T12 / T21 built as :364-370,
                      every row in the text's operation order, decisions exact;
  np_replay           the acceptance rule of iterate (:228-253) over a list of counts;
  the C ABI           symbols, struct mirrors, MCS_ERR_ARG before any device use,
                      MCS_ERR_NO_DEVICE on a machine without a GPU.

cv::eigen and cv::Rodrigues are OpenCV internals: a hypothesis is compared mathematically (stage
A), and only where the text defines it: three distinct indices and a relative gap above GAP
between the two largest eigenvalues of N.  Everything downstream of (s, R, t) is exact (stage B)
except a decision within MARGIN (relative) of maxerr, which is counted as unsure.
"""
import math
import os

import numpy as np
import pytest

from tests.test_fuse_ref import MARGIN, _inv_mat, _matmul_lr, make_rig, make_target

PROB, MIN_INL, CAP = 0.98, 15, 300        # the call site: SetRansacParameters(0.98, 15, 300)
GAP = 1e-3                                # stage A compares only above this relative eigenvalue gap
# Stage A: the largest difference between the eigh and the Jacobi restatement over every compared
# hypothesis of CASES below is 1.7331e-13 (test_stage_a_tolerance_is_ten_times_the_cpu_spread prints
# and bounds it); the device adds a different sweep order, sincos and atan2: 10 x.
CPU_SPREAD = 1.7331e-13
TOL_A = 10 * CPU_SPREAD


# ----------------------------------------------------------------------------- the restatement
def np_draw_samples(n, draws):
    """:202-222 with vAvailableIndices as a list of n that keeps popped values."""
    out = []
    for d in np.asarray(draws).reshape(-1, 3):
        v, size, tri = list(range(n)), n, []
        for randi in d:
            idx = v[int(randi)]
            tri.append(idx)
            v[idx] = v[size - 1]          # vAvailableIndices[idx] = back()
            size -= 1                     # pop_back()
        out.append(tri)
    return np.array(out, np.int32).reshape(-1, 3)


def _mat_vec_add(A, x, b):
    out = []
    for i in range(3):
        s = 0.0
        for k in range(3):
            s += float(A[i][k]) * float(x[k])
        out.append(s + float(b[i]))
    return out


def _w2i(cam, x, y, z):
    """cCamModelGeneral_::WorldToImg (src/cam_model_omni.cpp:147-163) on arrays, element by element
    in the text's order; cam = c d e u0 v0 invP[12]."""
    x, y, z = (np.asarray(a, np.float64) for a in (x, y, z))
    with np.errstate(all="ignore"):
        norm = np.sqrt(x * x + y * y)
        norm = np.where(norm == 0.0, 1e-14, norm)
        theta = np.arctan(-z / norm)
        rho = np.zeros_like(theta)
        for a in cam[5:17][::-1]:
            rho = rho * theta + float(a)
        uu, vv = x / norm * rho, y / norm * rho
        return uu * float(cam[0]) + vv * float(cam[1]) + float(cam[3]), uu * float(cam[2]) + vv + float(cam[4])


def _cam_hom(Mt, Mc, cam, X):
    """WorldToCamHom_fast (src/cam_system_omni.cpp:92-112): invMat(M_t M_c) * [X 1], WorldToImg."""
    inv = _inv_mat(_matmul_lr(Mt, Mc))
    pc = []
    for i in range(3):
        s = 0.0
        for k in range(3):
            s += float(inv[i, k]) * float(X[k])
        s += float(inv[i, 3]) * 1.0
        pc.append(s)
    u, v = _w2i(cam, pc[0], pc[1], pc[2])
    return float(u), float(v)


def np_prepare(rig, kf1, pts1, kf2, pts2, matches12, ok1, ok2, first1, first2, sigma2):
    """The constructor (:44-137) for one candidate -> dict of rows in i1 order."""
    Mt1, Mt2 = np.asarray(kf1["m_t"], np.float64).reshape(4, 4), np.asarray(kf2["m_t"], np.float64).reshape(4, 4)
    h1, h2 = _inv_mat(Mt1), _inv_mat(Mt2)
    r = dict(idx1=[], X1=[], X2=[], p1=[], p2=[], cam1=[], cam2=[], maxerr1=[], maxerr2=[])
    for i1 in range(len(matches12)):
        m = int(matches12[i1])
        if m < 0 or not ok1[i1] or not ok2[m]:
            continue
        f1, f2 = int(first1[i1]), int(first2[m])
        if f1 < 0 or f2 < 0:
            continue
        c1, c2 = int(kf1["kp_cam"][f1]), int(kf2["kp_cam"][f2])
        # mvnMaxError1 / 2 are std::vector<size_t> (include/cSim3Solver.h:92-93): push_back truncates
        r["maxerr1"].append(float(int(9.210 * float(sigma2[int(kf1["kp_octave"][f1])]))))
        r["maxerr2"].append(float(int(9.210 * float(sigma2[int(kf2["kp_octave"][f2])]))))
        r["idx1"].append(i1)
        Xa, Xb = pts1["pos"][i1], pts2["pos"][m]
        r["p1"].append(_cam_hom(Mt1, rig["m_c"][c1], rig["cam"][c1], Xa))
        r["X1"].append(_mat_vec_add(h1[:3, :3], Xa, h1[:3, 3]))
        r["cam1"].append(c1)
        r["p2"].append(_cam_hom(Mt2, rig["m_c"][c2], rig["cam"][c2], Xb))
        r["X2"].append(_mat_vec_add(h2[:3, :3], Xb, h2[:3, 3]))
        r["cam2"].append(c2)
    dt = dict(idx1=np.int32, cam1=np.int32, cam2=np.int32)
    w = dict(X1=3, X2=3, p1=2, p2=2)
    out = {k: np.array(v, dt.get(k, np.float64)).reshape((-1, w[k]) if k in w else (-1,)) for k, v in r.items()}
    out["n"] = len(r["idx1"])
    return out


def np_max_its(N, prob=PROB, min_inl=MIN_INL, cap=CAP):
    """:139-165 -> (mRansacMaxIts, the value before ceil or None).  N < min_inliers: 0 (iterate
    returns at :177, the text's value is never read)."""
    if N < min_inl:
        return 0, None
    if N == min_inl:
        return 1, None
    eps = float(min_inl) / N
    v = math.log(1 - prob) / math.log(1 - math.pow(eps, 3))
    return max(1, min(int(math.ceil(v)), cap)), v


def jacobi4(A):
    """Plain cyclic Jacobi on a symmetric 4x4 -> (eigenvalues, eigenvectors in columns)."""
    a, v = np.array(A, np.float64), np.eye(4)
    for _ in range(30):
        off = sum(abs(a[p, q]) for p in range(4) for q in range(p + 1, 4))
        if off <= 1e-18 * (off + sum(abs(a[p, p]) for p in range(4))):
            break
        for p in range(4):
            for q in range(p + 1, 4):
                if a[p, q] == 0.0:
                    continue
                th = (a[q, q] - a[p, p]) / (2.0 * a[p, q])
                t = math.copysign(1.0, th) / (abs(th) + math.sqrt(th * th + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                J = np.eye(4)
                J[p, p] = J[q, q] = c
                J[p, q], J[q, p] = s, -s
                a, v = J.T @ a @ J, v @ J
                a[p, q] = a[q, p] = 0.0
    return np.diag(a).copy(), v


def np_horn(X1, X2, tri, solver="eigh"):
    """computeT (:286-371) -> (s, R [3, 3], t [3], relative gap between the two largest
    eigenvalues of N).  cv::eigen -> eigh sorted descending (or jacobi4); cv::Rodrigues restated."""
    P1, P2 = np.asarray(X1, np.float64)[list(tri)].T.copy(), np.asarray(X2, np.float64)[list(tri)].T.copy()
    O1, O2 = P1.sum(1) * (1.0 / 3.0), P2.sum(1) * (1.0 / 3.0)
    Pr1, Pr2 = P1 - O1[:, None], P2 - O2[:, None]
    M = Pr2 @ Pr1.T
    N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                  [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                  [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                  [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]])
    N = N + np.triu(N, 1).T
    ev, evec = np.linalg.eigh(N) if solver == "eigh" else jacobi4(N)
    order = np.argsort(-ev, kind="stable")
    ev, q = ev[order], evec[:, order[0]]
    gap = (ev[0] - ev[1]) / max(np.abs(ev).max(), 1e-300)
    with np.errstate(all="ignore"):
        nv = math.sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
        ang = math.atan2(nv, q[0])
        rv = q[1:] * (2.0 * ang / nv) if nv != 0.0 else np.full(3, np.nan)
        th = math.sqrt(float(rv @ rv))
        if th < np.finfo(np.float64).eps:
            R = np.eye(3)
        else:
            x, y, z = rv / th
            c, s = math.cos(th), math.sin(th)
            K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
            R = c * np.eye(3) + (1 - c) * np.outer([x, y, z], [x, y, z]) + s * K
        P3 = R @ Pr2
        sc = float((Pr1 * P3).sum() / (P3 * P3).sum())
        t = O1 - sc * (R @ O2)
    return sc, R, t, float(gap)


def srt_diff(a, b):
    """The stage-A measure between two (s, R, t): relative in s, absolute in R, relative to 1 + |t| in t."""
    return max(abs(a[0] - b[0]) / abs(b[0]), float(np.abs(np.asarray(a[1]) - b[1]).max()),
               float(np.abs(np.asarray(a[2]) - b[2]).max()) / (1.0 + float(np.abs(b[2]).max())))


def np_transforms(s, R, t):
    """:364-370 from (s, R, t): sR, sRinv = (1.0 / s) * R.t(), tinv = -sRinv * t."""
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    with np.errstate(all="ignore"):
        sR, sRi = R * float(s), R.T * (1.0 / float(s))
        neg = sRi * -1.0
        tinv = np.array([(0.0 + neg[i, 0] * t[0] + neg[i, 1] * t[1]) + neg[i, 2] * t[2] for i in range(3)])
    return sR, t, sRi, tinv


def _hom(A, b, X):
    """Rows 0..2 of [A b; 0 0 0 1] * (X, 1) for rows of X: s = 0; s += a(i,k) x(k), k = 0..3."""
    with np.errstate(all="ignore"):
        return [((0.0 + A[i][0] * X[0] + A[i][1] * X[1]) + A[i][2] * X[2]) + b[i] * 1.0 for i in range(3)]


def np_check(rig, rows, s, R, t):
    """CheckInliers (:374-415) -> (inlier bool [N], unsure bool [N], fail1 bool [N], fail2 bool [N])."""
    N = rows["n"]
    if N == 0:
        z = np.zeros(0, bool)
        return z, z, z, z
    sR, t, sRi, tinv = np_transforms(s, R, t)
    X1, X2 = rows["X1"].T, rows["X2"].T
    p21, p12 = _hom(sR, t, X2), _hom(sRi, tinv, X1)
    e1, e2 = np.zeros(N), np.zeros(N)
    for c in range(len(rig["m_c"])):
        im = _inv_mat(np.asarray(rig["m_c"][c], np.float64).reshape(4, 4))
        cam = np.asarray(rig["cam"][c], np.float64)
        for err, pt, cams, p, sign in ((e1, p21, rows["cam1"], rows["p1"], 1.0), (e2, p12, rows["cam2"], rows["p2"], -1.0)):
            k = cams == c
            if not k.any():
                continue
            q = _hom(im[:3, :3], im[:3, 3], [a[k] for a in pt])
            u, v = _w2i(cam, q[0], q[1], q[2])
            with np.errstate(all="ignore"):
                dx, dy = (p[k, 0] - u) * sign, (p[k, 1] - v) * sign
                err[k] = dx * dx + dy * dy
    with np.errstate(all="ignore"):
        ok1, ok2 = e1 < rows["maxerr1"], e2 < rows["maxerr2"]
        unsure = (np.abs(e1 - rows["maxerr1"]) <= MARGIN * rows["maxerr1"]) | \
                 (np.abs(e2 - rows["maxerr2"]) <= MARGIN * rows["maxerr2"])
    return ok1 & ok2, unsure, ~ok1 & ok2, ok1 & ~ok2


def np_replay(counts, iterations, best, max_its, min_inl=MIN_INL):
    """:196-253 over the counts of the iterations a call evaluates -> (success, no_more, iterations
    after, best_inliers after, index of the hypothesis the best values come from or None)."""
    kbest = None
    for k, inl in enumerate(counts):
        iterations += 1
        if inl >= best:
            best, kbest = inl, k
            if inl > min_inl:
                return True, False, iterations, best, kbest
    return False, iterations >= max_its, iterations, best, kbest


# ----------------------------------------------------------------------------- scripted inputs
def sigma2_of(rig):
    return np.asarray(rig["scale"], np.float64) ** 2


def make_solver_case(seed, Ns=(50,), n_per_cam=60, inlier=(0.6,), n_skip=6, n_its=CAP):
    """KF1 and len(Ns) candidates on the Lafida rig, candidate t with exactly Ns[t] correspondences
    after the constructor's skip rules plus n_skip matches that each rule drops.  A share
    `inlier[t]` of the pairs is the same place under the candidate's Sim3 (a little noise), a
    share is off by a few pixels (fails one of the two tests where the octaves differ) and the
    rest is elsewhere.  Some matched points observe their keyframe at another keypoint than their
    slot (first != slot).  -> dict."""
    rng = np.random.default_rng(seed)
    rig = make_rig(3)
    kf1 = make_target(rig, rng, n_per_cam, 32, False)
    n1 = len(kf1["kp_xy"])
    assert n1 >= max(Ns) + n_skip + 4
    pos1 = np.zeros((n1, 3))
    for i in range(n1):
        M = kf1["m_t"] @ rig["m_c"][int(kf1["kp_cam"][i])]
        pos1[i] = M[:3, :3] @ (kf1["rays"][i] * rng.uniform(0.8, 6.0)) + M[:3, 3]
    pts1 = dict(pos=pos1, dist=np.ones((n1, 2)), desc=np.zeros((n1, 32), np.uint8), mask=None)
    ok1 = np.ones(n1, np.uint8)
    first1 = np.arange(n1, dtype=np.int32)
    for i in rng.choice(n1, n1 // 5, replace=False):          # observed first at another keypoint
        first1[i] = int(rng.integers(n1))
    dead = rng.choice(n1, 4, replace=False)                  # KF1's own skip rules: !ok1 and first1 < 0
    ok1[dead[:2]] = 0
    first1[dead[2:]] = -1
    live = np.setdiff1d(np.arange(n1), dead)
    T1 = np.linalg.inv(kf1["m_t"])
    from tests.test_sim3_ref import cayley_rot
    kf2s, pts2s, ok2s, first2s, m12, sims = [], [], [], [], np.full((len(Ns), n1), -1, np.int32), []
    for t, N in enumerate(Ns):
        kf2 = make_target(rig, rng, n_per_cam, 32, False)
        n2 = len(kf2["kp_xy"])
        s12, R12, t12 = float(rng.uniform(0.7, 1.5)), cayley_rot(rng.uniform(-0.06, 0.06, 3)), rng.uniform(-0.2, 0.2, 3)
        pos2 = rng.normal(0, 3.0, (n2, 3))
        ok2, first2 = np.ones(n2, np.uint8), np.arange(n2, dtype=np.int32)
        for k in rng.choice(n2, n2 // 5, replace=False):
            first2[k] = int(rng.integers(n2))
        i1s = np.concatenate([rng.choice(live, N + n_skip, replace=False), dead])
        i2s = rng.choice(n2, N + n_skip + 4, replace=False)
        frac = inlier[t % len(inlier)]
        for i1, i2 in zip(i1s, i2s):
            m12[t, i1] = i2
            p1 = T1[:3, :3] @ pos1[i1] + T1[:3, 3]
            p2 = (R12.T @ (p1 - t12)) / s12
            d = float(np.linalg.norm(p2))
            u = rng.random()
            noise = 0.0004 if u < frac else 0.012 if u < frac + 0.5 * (1 - frac) else 0.5
            p2 = p2 + rng.normal(0, noise * d, 3)
            pos2[i2] = kf2["m_t"][:3, :3] @ p2 + kf2["m_t"][:3, 3]
        for j, i2 in enumerate(i2s[N:N + n_skip]):           # the candidate's skip rules, in turn
            if j % 2 == 0:
                ok2[i2] = 0
            else:
                first2[i2] = -1
        kf2s.append(kf2)
        pts2s.append(dict(pos=pos2, dist=np.ones((n2, 2)), desc=np.zeros((n2, 32), np.uint8), mask=None))
        ok2s.append(ok2)
        first2s.append(first2)
        sims.append((s12, R12, t12))
    sigma2 = sigma2_of(rig)
    case = dict(rig=rig, kf1=kf1, pts1=pts1, kf2s=kf2s, pts2s=pts2s, matches12=m12, ok1=ok1, ok2s=ok2s,
                first1=first1, first2s=first2s, sigma2=sigma2, sims=sims)
    case["rows"] = [np_prepare(rig, kf1, pts1, kf2s[t], pts2s[t], m12[t], ok1, ok2s[t], first1, first2s[t], sigma2)
                    for t in range(len(Ns))]
    assert [r["n"] for r in case["rows"]] == list(Ns)
    draws = [rng.integers(0, max(r["n"], 3), (n_its, 3)) for r in case["rows"]]
    case["draws"] = draws
    case["samples"] = np.stack([np_draw_samples(max(r["n"], 3), d) if r["n"] >= 3 else np.zeros((n_its, 3), np.int32)
                                for r, d in zip(case["rows"], draws)]).astype(np.int32)
    # repeats are rare among the draws of a large N (about 2 / N^2 per iteration): two are scripted
    # in, by draws that read position N - 1 again after it was popped
    for t, r in enumerate(case["rows"]):
        if np_max_its(r["n"])[0] >= 50:
            N, b = r["n"], int(rng.integers(r["n"] - 2))
            draws[t][1], draws[t][2] = (N - 1, N - 1, b), (N - 1, N - 1, N - 1)   # -> (N-1, N-1, b), (N-1, N-1, N-2)
            case["samples"][t][1:3] = np_draw_samples(N, draws[t][1:3])
    return case


def np_good_flags(case, seed):
    """The caller's `has a good map point` flags for the hand-over: mostly set."""
    rng = np.random.default_rng(seed)
    n1 = len(case["kf1"]["kp_xy"])
    return (rng.random(n1) < 0.9).astype(np.uint8), [(rng.random(len(k["kp_xy"])) < 0.9).astype(np.uint8)
                                                      for k in case["kf2s"]]


def np_active(case, inlier, good1, good2s):
    """src/cORBmatcher.cpp:1758-1774 with vpMatches12 = the inliers' entries (cLoopClosing.cpp:354-360)."""
    from tests.test_sim3_ref import np_sim3_active
    a1, a2 = [], []
    for t in range(len(case["kf2s"])):
        m = np.where(inlier[t] != 0, case["matches12"][t], -1)
        f = np.array([case["first2s"][t][k] if k >= 0 else -1 for k in m])
        z1, z2 = np.zeros(len(good1), bool), np.zeros(len(good2s[t]), bool)
        r = np_sim3_active(good1 != 0, z1, good2s[t] != 0, z2, m, f)
        a1.append(r[0])
        a2.append(r[1])
    return np.stack(a1), a2


def np_solve(case, t, n_call, state=None, solver="eigh"):
    """One iterate(n_call) of candidate t entirely in NumPy -> dict (state after, outputs, per
    hypothesis srt [k, 13], counts, checks)."""
    rows = case["rows"][t]
    N = rows["n"]
    st = dict(state) if state else dict(iterations=0, best=0, max_its=np_max_its(N)[0], best_k=None)
    k0, k1 = st["iterations"], min(st["iterations"] + n_call, st["max_its"])
    srt, checks = [], []
    for k in range(k0, k1):
        s, R, tt, gap = np_horn(rows["X1"], rows["X2"], case["samples"][t][k], solver)
        srt.append(np.concatenate([[s], R.ravel(), tt]))
        checks.append(np_check(case["rig"], rows, s, R, tt))
    counts = [int(c[0].sum()) for c in checks]
    ok, no_more, its, best, kb = np_replay(counts, k0, st["best"], st["max_its"])
    return dict(success=ok, no_more=no_more, iterations=its, best=best, max_its=st["max_its"], kbest=kb,
                khit=kb if ok else None, srt=np.array(srt).reshape(-1, 13), counts=counts, checks=checks, first=k0)


# ----------------------------------------------------------------------------- tests (no GPU)
NEW_SYMBOLS = ["mcs_sim3_draw_samples", "mcs_sim3_solver_workspace_create", "mcs_sim3_solver_workspace_destroy",
               "mcs_sim3_solver_prepare_device", "mcs_sim3_solver_iterate_device", "mcs_sim3_solver_active_device",
               "mcs_sim3_solver"]
CASES = {"t1_n50": dict(seed=11, Ns=(50,), inlier=(0.55,)),
         "t3_mixed": dict(seed=12, Ns=(65, 16, 129), n_per_cam=70, inlier=(0.5, 0.6, 0.45)),
         "t3_small": dict(seed=13, Ns=(14, 15, 63), inlier=(0.6,))}
# The boundary counts of the check kernel and of max_its, each as candidate 0 of a batch of three
# whose companions (N = 40 with enough inliers, N = 20 with too few) make every batch show a late
# hit and a candidate without one.  The seeds are checked on the CPU by
# test_boundary_batches_are_not_vacuous (coverage, no unsure decision, stage-A exclusions).
BOUNDARY = {0: 101, 14: 240, 15: 250, 16: 260, 63: 730, 64: 740, 65: 750, 129: 1390}
# The check kernel stages the correspondences in chunks of 256 (one below, at, one above, and a
# third chunk); the prepare kernel walks the slots and moves the rows in rounds of 1024: N = 1030 of
# 1110 slots is a second slot round, a second row round and a fifth chunk.
BOUNDARY.update({255: 2550, 256: 2560, 257: 2570, 513: 5130, 1030: 10302})
PER_CAM = {255: 200, 256: 200, 257: 200, 513: 200, 1030: 370}          # keypoints per camera where 60 cannot hold N
K_CHUNK, K_PREP = 256, 1024
_CACHE = {}


def get_case(name):
    if name not in _CACHE:
        _CACHE[name] = make_solver_case(**CASES[name])
    return _CACHE[name]


def boundary_case(N):
    if ("b", N) not in _CACHE:
        _CACHE["b", N] = make_solver_case(seed=BOUNDARY[N], Ns=(N, 40, 20), n_per_cam=PER_CAM.get(N, 60),
                                          inlier=(0.55, 0.55, 0.3))
    return _CACHE["b", N]


def test_new_symbols_exported_and_registered(built):
    import mcs_amd
    L = mcs_amd.lib()
    for s in NEW_SYMBOLS:
        assert s in mcs_amd.SIGNATURES, s
        assert hasattr(L, s), s


@pytest.mark.parametrize("name,cls", [("mcs_sim3_corr", "Sim3Corr"), ("mcs_sim3_ransac", "Sim3Ransac")])
def test_structs_match_the_header(name, cls):
    import re
    import mcs_amd
    from mcs_amd import sim3_solver
    txt = open(os.path.join(mcs_amd.INCLUDE_DIR, "mcs_matcher.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        fields += re.findall(r"(\w+)\s*(?:,|$)", decl.strip())
    assert fields == [f[0] for f in getattr(sim3_solver, cls)._fields_]


def test_draw_quirks_by_hand():
    """n = 5.  Draws (1, 1, 1): idx 1; v[1] = v[4] = 4; idx 4; v[4] = v[3] = 3; then v[1] is still 4:
    a repeated index.  Draws (4, 4, 4): idx 4, v[4] = v[4]; the second draw reads position 4, which
    is past the shrunk vector (size 4) and still holds 4; v[4] = v[3] = 3; third reads 3."""
    assert np_draw_samples(5, [[1, 1, 1]]).tolist() == [[1, 4, 4]]
    assert np_draw_samples(5, [[4, 4, 4]]).tolist() == [[4, 4, 3]]
    assert np_draw_samples(5, [[0, 1, 2]]).tolist() == [[0, 1, 2]]
    assert np_draw_samples(5, [[0, 0, 0]]).tolist() == [[0, 4, 4]]        # the swap went to the value 0 = position 0


def test_draw_helper_equals_the_restatement(built):
    from mcs_amd import sim3_solver as ss
    rng = np.random.default_rng(5)
    n_rep = n_past = 0
    for n in (3, 4, 5, 15, 16, 64, 129, 1000):
        d = rng.integers(0, n, (400, 3))
        want = np_draw_samples(n, d)
        assert np.array_equal(ss.draw_samples(n, d), want)
        assert ((want >= 0) & (want < n)).all()
        n_rep += int(((want[:, 0] == want[:, 1]) | (want[:, 1] == want[:, 2]) | (want[:, 0] == want[:, 2])).sum())
        n_past += int((d[:, 1] >= n - 1).sum() + (d[:, 2] >= n - 2).sum())
    assert n_rep > 50 and n_past > 50
    assert np.array_equal(ss.draw_samples(5, [[1, 1, 1], [4, 4, 4]]), [[1, 4, 4], [4, 4, 3]])


def test_draw_helper_argument_errors(built):
    import mcs_amd
    from mcs_amd import sim3_solver as ss
    for n, d in ((2, [[0, 1, 0]]), (5, [[0, 5, 1]]), (5, [[-1, 0, 1]])):
        with pytest.raises(mcs_amd.McsError) as e:
            ss.draw_samples(n, d)
        assert e.value.code == mcs_amd.MCS_ERR_ARG


FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sim3solver_ref.npz")


def test_max_its_equals_the_reference_text():
    """tests/golden/sim3solver_ref.npz: SetRansacParameters evaluated from the reference text for
    N = 15 .. 200 and a few larger counts, under the call site's parameters and the constructor's
    defaults.  np_max_its must give the same, and the value before ceil keeps 1e-9 from an integer."""
    f = np.load(FIX)
    assert f["n_statements"] > 5
    for (prob, mn, cap), row in zip(f["params"], f["max_its"]):
        for N, want in zip(f["n_list"], row):
            if want < 0:
                continue
            got, v = np_max_its(int(N), float(prob), int(mn), int(cap))
            assert got == want, (N, prob, got, want)
            assert v is None or abs(v - round(v)) > 1e-9
    assert f["max_its"][0][list(f["n_list"]).index(50)] == 143


def load_ctor_scenario(seed):
    """A constructor scenario of the fixture as the arrays the library takes -> case dict (T = 1)
    and the text's rows."""
    f = np.load(FIX)
    p = "ctor%d_" % seed
    rig = make_rig(3)
    kfs, pts, ok, first = [], [], [], []
    for tag in ("k1_", "k2_"):
        n = len(f[p + tag + "kp_cam"])
        kfs.append(dict(kp_xy=f[p + tag + "kp_xy"], kp_octave=f[p + tag + "kp_octave"], kp_cam=f[p + tag + "kp_cam"],
                        m_t=f[p + tag + "m_t"], desc=np.zeros((n, 32), np.uint8), mask=None, rays=None))
        sl = f[p + tag + "slots"]
        pts.append(dict(pos=np.where(sl[:, None] >= 0, f[p + "pos"][np.maximum(sl, 0)], 0.0), dist=np.ones((n, 2)),
                        desc=np.zeros((n, 32), np.uint8), mask=None))
        ok.append(((sl >= 0) & (f[p + "mp_bad"][np.maximum(sl, 0)] == 0)).astype(np.uint8))
        first.append(f[p + tag + "first"].astype(np.int32))
    case = dict(rig=rig, kf1=kfs[0], pts1=pts[0], kf2s=[kfs[1]], pts2s=[pts[1]], matches12=f[p + "matches12"][None].copy(),
                ok1=ok[0], ok2s=[ok[1]], first1=first[0], first2s=[first[1]], sigma2=f[p + "sigma2"],
                slots=(f[p + "k1_slots"], f[p + "k2_slots"]))
    want = {k: f[p + k] for k in ("idx1", "cam1", "cam2", "maxerr1", "maxerr2", "X1", "X2", "p1", "p2", "all")}
    want["n"], want["max_its_default"] = int(f[p + "N"]), int(f[p + "max_its"])
    return case, want


CTOR_SEEDS = (901, 902)


def same_as_text(rows, want, p_tol=0.0):
    n = want["n"]
    assert rows["n"] == n
    for k in ("idx1", "cam1", "cam2", "maxerr1", "maxerr2", "X1", "X2"):
        assert np.array_equal(np.asarray(rows[k])[:n], want[k]), k
    for k in ("p1", "p2"):
        assert np.abs(np.asarray(rows[k])[:n] - want[k]).max(initial=0.0) <= p_tol, k


@pytest.mark.parametrize("seed", CTOR_SEEDS)
def test_constructor_restatement_equals_the_reference_text(seed):
    """The constructor (:44-137) evaluated from the reference text on a scripted map: np_prepare gives
    the same rows bit for bit, and the scenario takes every skip rule."""
    c, want = load_ctor_scenario(seed)
    rows = np_prepare(c["rig"], c["kf1"], c["pts1"], c["kf2s"][0], c["pts2s"][0], c["matches12"][0], c["ok1"], c["ok2s"][0],
                      c["first1"], c["first2s"][0], c["sigma2"])
    same_as_text(rows, want)
    assert np.array_equal(want["all"], np.arange(want["n"]))                 # mvAllIndices is the identity
    assert want["max_its_default"] == np_max_its(want["n"], 0.99, 6, 300)[0]  # the constructor's own SetRansacParameters()
    m, kept = c["matches12"][0], set(int(i) for i in want["idx1"])
    matched = np.flatnonzero(m >= 0)
    sl1, sl2 = c["slots"]
    why = {"null_or_bad_pMP1": 0, "bad_pMP2": 0, "first1_negative": 0, "first2_negative": 0}
    for i in matched:
        if i in kept:
            continue
        if not c["ok1"][i]:
            why["null_or_bad_pMP1"] += 1
        elif not c["ok2s"][0][m[i]]:
            why["bad_pMP2"] += 1
        elif c["first1"][i] < 0:
            why["first1_negative"] += 1
        else:
            assert c["first2s"][0][m[i]] < 0
            why["first2_negative"] += 1
    assert all(v >= 1 for v in why.values()), why
    assert any(c["first1"][i] != i for i in kept) and any(c["first2s"][0][m[i]] != m[i] for i in kept)


ITER_CASES = [("t3_mixed", 0), ("t3_mixed", 1), ("t3_mixed", 2), ("t3_small", 0), ("t3_small", 1), ("t3_small", 2)]


def load_iterate(name, t):
    f = np.load(FIX)
    p = "it_%s_%d_" % (name, t)
    return {k: f[p + k] for k in ("N", "max_its", "visits", "vbInliers", "best", "P1", "P2", "srt", "inl", "cnt")}


def text_events(name, t):
    """What the text's run of a candidate shows -> set of scenario names."""
    x, c = load_iterate(name, t), get_case(name)
    ev, best = set(), 0
    for ok, no_more, n_inl, its, b in x["visits"]:
        if ok and its > 1 and "hit" not in ev:
            ev.add("hit_after_failing_iterations")
        if ok and "hit" in ev and n_inl == best:
            ev.add("tie_after_a_success")
        if ok:
            ev.add("hit")
        if no_more:
            ev.add("ran_to_no_more")
        best = b
    E, N = len(x["cnt"]), int(x["N"])
    tri, d = c["samples"][t][:E], c["draws"][t][:E]
    if ((tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2])).any():
        ev.add("repeated_index_triple")
    if ((d[:, 1] >= N - 1) | (d[:, 2] >= N - 2)).any():
        ev.add("draw_past_the_shrunk_vector")
    ev.add("N_%d" % N)
    return ev


def test_text_runs_show_the_named_scenarios():
    ev = set().union(*[text_events(n, t) for n, t in ITER_CASES])
    want = {"hit_after_failing_iterations", "ran_to_no_more", "N_15", "N_14", "draw_past_the_shrunk_vector",
            "repeated_index_triple", "tie_after_a_success"}
    assert want <= ev, want - ev


@pytest.mark.parametrize("name,t", ITER_CASES)
def test_iterate_restatement_equals_the_reference_text(name, t):
    """iterate, centroid, computeT and CheckInliers evaluated from the reference text in six visits of
    50 (tests/golden/gen_sim3solver_ref.py): the draws select the same correspondences (exact), the
    hypotheses agree to the stage-A tolerance where the text defines them, CheckInliers from the text's
    own (s, R, t) gives the same decisions (exact), and the replay of the acceptance rule gives every
    visit's return value, bNoMore, nInliers, mnIterations, mnBestInliers, vbInliers and mBest*."""
    x, c = load_iterate(name, t), get_case(name)
    rows, N, E = c["rows"][t], int(x["N"]), len(x["cnt"])
    assert N == rows["n"] and x["max_its"] == np_max_its(N)[0]
    tri = c["samples"][t][:E]
    assert np.array_equal(tri, np_draw_samples(max(N, 3), c["draws"][t][:E])) or E == 0
    checks, n_cmp = [], 0
    for k in range(E):
        assert np.array_equal(x["P1"][k], rows["X1"][tri[k]].T) and np.array_equal(x["P2"][k], rows["X2"][tri[k]].T)   # draws
        h = x["srt"][k]
        if len(set(int(i) for i in tri[k])) == 3:
            ref = np_horn(rows["X1"], rows["X2"], tri[k])
            if ref[3] > GAP:
                n_cmp += 1
                assert srt_diff((h[0], h[1:10].reshape(3, 3), h[10:13]), ref) <= TOL_A, k
        inl, unsure, _, _ = np_check(c["rig"], rows, h[0], h[1:10].reshape(3, 3), h[10:13])
        assert unsure.sum() == 0
        assert np.array_equal(inl, x["inl"][k] != 0) and inl.sum() == x["cnt"][k], k               # decisions
        checks.append(inl)
    assert E - n_cmp <= max(0.1 * E, 2)
    its, best, k0, last = 0, 0, 0, None
    mx = np_max_its(N)[0]
    for v, (ok, no_more, n_inl, its_after, best_after) in enumerate(x["visits"]):
        nv = max(min(50, mx - its), 0)
        got = np_replay([int(cnt) for cnt in x["cnt"][k0:k0 + nv]], its, best, mx)
        used = got[2] - its
        assert (int(got[0]), int(got[1]), got[2], got[3]) == (ok, no_more, its_after, best_after), v
        if got[4] is not None:
            last = k0 + got[4]
        want_inl = np.zeros(x["vbInliers"].shape[1], np.uint8)
        if ok:
            assert n_inl == x["cnt"][last]
            want_inl[rows["idx1"][checks[last]]] = 1
        else:
            assert n_inl == 0
        assert np.array_equal(x["vbInliers"][v], want_inl)
        if last is not None:
            h = x["srt"][last]
            sR, tt, _, _ = np_transforms(h[0], h[1:10], h[10:13])
            T12 = np.eye(4)
            T12[:3, :3], T12[:3, 3] = sR, tt
            assert np.array_equal(x["best"][v][:13], h, equal_nan=True)
            assert np.array_equal(x["best"][v][13:29], T12.ravel(), equal_nan=True)
            if ok:
                assert np.array_equal(x["best"][v][29:45], T12.ravel(), equal_nan=True)
        its, best, k0 = got[2], got[3], k0 + used
    assert k0 == E


def test_max_error_vectors_hold_integers_in_the_text():
    """include/cSim3Solver.h declares mvnMaxError1 / 2 as std::vector<size_t>: the constructor's
    push_back(9.210 * sigma2) truncates, which np_prepare and the kernel reproduce."""
    f = np.load(FIX)
    kind = dict(zip(f["vectors"], f["vector_is_integral"]))
    assert kind["mvnMaxError1"] == 1 and kind["mvnMaxError2"] == 1 and kind["mvnIndices1"] == 1
    c = get_case("t1_n50")
    for k in ("maxerr1", "maxerr2"):
        assert np.array_equal(c["rows"][0][k], np.floor(c["rows"][0][k]))
    assert (np.floor(9.210 * c["sigma2"]) != 9.210 * c["sigma2"]).all()          # the truncation is never a no-op


def test_fixture_regenerates_from_reference_text(tmp_path):
    ref = "/root/reference"
    if not os.path.isdir(ref):
        pytest.skip("no reference checkout on this machine")
    import subprocess
    import sys
    out = str(tmp_path / "again.npz")
    subprocess.check_call([sys.executable, os.path.join(os.path.dirname(FIX), "gen_sim3solver_ref.py"), "--ref", ref,
                           "--out", out])
    a, b = np.load(FIX), np.load(out)
    assert sorted(a.files) == sorted(b.files) and all(np.array_equal(a[k], b[k]) for k in a.files)


def test_max_its_values_and_margin():
    """143 at N = 50 (below the cap), the cap from N = 64 on, 1 at N == min, 0 below; the value
    before ceil is farther than 1e-9 from an integer on every N the tests use."""
    assert np_max_its(50)[0] == 143 and np_max_its(63)[0] == 288 and np_max_its(64)[0] == CAP
    assert np_max_its(15) == (1, None) and np_max_its(14) == (0, None) and np_max_its(16)[0] == 3
    for N in (16, 50, 63, 64, 65, 129, 150):
        v = np_max_its(N)[1]
        assert abs(v - round(v)) > 1e-9


def test_constructor_uses_the_first_observation():
    """Octave, camera and projection come from keypoint `first`, the position from the slot."""
    c = get_case("t1_n50")
    rows, kf1, kf2 = c["rows"][0], c["kf1"], c["kf2s"][0]
    assert rows["n"] == 50
    moved1 = [i for i, i1 in enumerate(rows["idx1"]) if c["first1"][i1] != i1]
    moved2 = [i for i, i1 in enumerate(rows["idx1"]) if c["first2s"][0][c["matches12"][0][i1]] != c["matches12"][0][i1]]
    assert len(moved1) >= 3 and len(moved2) >= 3
    for i in moved1:
        f = c["first1"][rows["idx1"][i]]
        assert rows["cam1"][i] == kf1["kp_cam"][f]
        assert rows["maxerr1"][i] == int(9.210 * c["sigma2"][kf1["kp_octave"][f]])
    for i in moved2:
        f = c["first2s"][0][c["matches12"][0][rows["idx1"][i]]]
        assert rows["cam2"][i] == kf2["kp_cam"][f]
    assert (np.diff(rows["idx1"]) > 0).all()
    assert (c["matches12"][0] >= 0).sum() > rows["n"]          # the skip rules dropped matches


def coverage(case, sols):
    """What a randomised case must show: a hit that is not iteration 0, a candidate without a hit,
    rows failing only err1 / only err2, a skipped match."""
    late = any(s["success"] and s["khit"] + s["first"] > 0 for s in sols)
    none = any(not s["success"] for s in sols)
    f1 = sum(int(c[2].sum()) for s in sols for c in s["checks"])
    f2 = sum(int(c[3].sum()) for s in sols for c in s["checks"])
    skipped = any((case["matches12"][t] >= 0).sum() > case["rows"][t]["n"] for t in range(len(sols)))
    return late, none, f1 > 0, f2 > 0, skipped


def test_n50_case_has_no_unsure_decision_and_143_iterations():
    c = get_case("t1_n50")
    s = np_solve(c, 0, CAP)
    assert s["max_its"] == 143 and sum(int(ch[1].sum()) for ch in s["checks"]) == 0 and excluded_within_limit(c)
    assert all(coverage(c, [s])[2:])                           # err1 only, err2 only, a skipped match


@pytest.mark.parametrize("name", ["t3_mixed", "t3_small"])
def test_cases_are_not_vacuous_and_have_no_unsure_decision(name):
    c = get_case(name)
    sols = [np_solve(c, t, CAP) for t in range(len(c["kf2s"]))]
    assert all(coverage(c, sols)), coverage(c, sols)
    assert sum(int(ch[1].sum()) for s in sols for ch in s["checks"]) == 0
    # a triple with a repeated index is evaluated by find, and a draw that reads past the shrunk
    # vector by the visits of 50 that go on to max_its
    rep = past = 0
    for t, s in enumerate(sols):
        tri, d, N = c["samples"][t][:s["iterations"]], c["draws"][t][:s["max_its"]], c["rows"][t]["n"]
        rep += int(((tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2])).sum())
        past += int(((d[:, 1] >= N - 1) | (d[:, 2] >= N - 2)).sum())
    assert rep >= 1 and past >= 1
    if name == "t3_small":
        assert [s["max_its"] for s in sols] == [0, 1, 288]
        assert sols[0]["no_more"] and not sols[0]["success"] and sols[0]["iterations"] == 0
        assert sols[1]["no_more"] and sols[1]["iterations"] == 1


def excluded_within_limit(case):
    """At most 10 % of a candidate's hypotheses fall outside stage A (one of up to three)."""
    for t, rows in enumerate(case["rows"]):
        mx = np_max_its(rows["n"])[0]
        if mx and (~stage_a_mask(case, t, 0, mx)).sum() > max(0.1 * mx, 0 if mx > 3 else 1):
            return False
    return True


@pytest.mark.parametrize("N", sorted(BOUNDARY))
def test_boundary_batches_are_not_vacuous(N):
    c = boundary_case(N)
    assert [r["n"] for r in c["rows"]] == [N, 40, 20]
    sols = [np_solve(c, t, CAP) for t in range(3)]
    assert all(coverage(c, sols)), coverage(c, sols)
    assert sum(int(ch[1].sum()) for s in sols for ch in s["checks"]) == 0
    assert excluded_within_limit(c)
    assert [s["max_its"] for s in sols][1:] == [np_max_its(40)[0], np_max_its(20)[0]]
    if N > K_PREP:
        # kept rows from slots on both sides of slot 1024; matched slots dropped below it, so the row
        # offset carried into the second slot round is not the slot offset, and at or above it, so
        # the second round compacts as well
        idx1, m = c["rows"][0]["idx1"], c["matches12"][0]
        assert (idx1 < K_PREP).any() and (idx1 >= K_PREP).any()
        dropped = np.setdiff1d(np.flatnonzero(m >= 0), idx1)
        assert (dropped >= K_PREP).any() and (dropped < K_PREP).any(), dropped
        assert len(m) > K_PREP and (N + K_CHUNK - 1) // K_CHUNK == 5


N_SINGLE = 40       # visits of one iteration: enough that the two scripted repeats stay under 10 %


def test_single_iteration_visits_are_not_vacuous():
    """N_SINGLE visits of one iteration on t3_mixed, as the GPU test makes them."""
    c = get_case("t3_mixed")
    sols = []
    for t in range(3):
        st, per = None, []
        for _ in range(N_SINGLE):
            o = np_solve(c, t, 1, st)
            per.append(o)
            st = dict(iterations=o["iterations"], best=o["best"], max_its=o["max_its"])
        sols.append(per)
    flat = [x for per in sols for x in per]
    assert any(x["success"] and x["khit"] + x["first"] > 0 for x in flat)
    assert any(not any(x["success"] for x in per) for per in sols)
    assert any(ch[2].any() for x in flat for ch in x["checks"]) and any(ch[3].any() for x in flat for ch in x["checks"])
    assert sum(int(ch[1].sum()) for x in flat for ch in x["checks"]) == 0
    n_eval = sum(len(x["counts"]) for x in flat)
    n_out = sum(int((~stage_a_mask(c, t, 0, per[-1]["iterations"])).sum()) for t, per in enumerate(sols))
    assert n_out <= 0.1 * n_eval, (n_out, n_eval)


def stage_a_mask(case, t, k0, k1):
    """Which hypotheses stage A compares: three distinct indices and a gap above GAP."""
    rows = case["rows"][t]
    keep = []
    for k in range(k0, k1):
        tri = case["samples"][t][k]
        keep.append(len(set(int(x) for x in tri)) == 3 and np_horn(rows["X1"], rows["X2"], tri)[3] > GAP)
    return np.array(keep, bool)


def test_stage_a_tolerance_is_ten_times_the_cpu_spread():
    """eigh against the plain Jacobi on every compared hypothesis of the cases; at most 10 % of
    the hypotheses of any candidate are excluded."""
    worst = 0.0
    for name in CASES:
        c = get_case(name)
        for t, rows in enumerate(c["rows"]):
            mx = np_max_its(rows["n"])[0]
            if mx == 0:
                continue
            keep = stage_a_mask(c, t, 0, mx)
            assert (~keep).sum() <= max(0.1 * mx, 0 if mx > 3 else 1), (name, t, int((~keep).sum()), mx)
            for k in np.flatnonzero(keep):
                a = np_horn(rows["X1"], rows["X2"], c["samples"][t][k], "eigh")
                b = np_horn(rows["X1"], rows["X2"], c["samples"][t][k], "jacobi")
                worst = max(worst, srt_diff(a, b))
    print("largest eigh / Jacobi difference: %.3g" % worst)
    assert worst <= CPU_SPREAD


def test_degenerate_triple_gives_nan_and_no_inliers():
    """Three times the same point with an exact centroid: Pr = 0, N = 0, den == 0.  s is 0 / 0 and
    every comparison of CheckInliers fails."""
    c = get_case("t1_n50")
    rows = c["rows"][0]
    X = np.zeros((3, 3))
    s, R, t, gap = np_horn(X, X, (0, 1, 2))
    assert np.isnan(s) and gap == 0.0
    assert np_check(c["rig"], rows, s, R, t)[0].sum() == 0
    assert np_check(c["rig"], rows, np.nan, np.full((3, 3), np.nan), np.full(3, np.nan))[0].sum() == 0


def test_replay_rule():
    """Ties take the later iteration; a hit needs > min; after a hit a tie with the best hits again."""
    assert np_replay([3, 5, 5, 4], 0, 0, 10) == (False, False, 4, 5, 2)
    assert np_replay([3, 16, 20], 0, 0, 10) == (True, False, 2, 16, 1)
    assert np_replay([15, 14], 0, 0, 2) == (False, True, 2, 15, 0)
    assert np_replay([12, 16, 17], 2, 16, 10) == (True, False, 4, 16, 1)     # the second iterate after a success


# ----------------------------------------------------------------------------- the C ABI without a GPU
def _host_call(edit=None, **kw):
    import mcs_amd
    from mcs_amd import sim3_solver as ss
    c = get_case("t1_n50")
    args = dict(matches12=c["matches12"], n_iterations=50, prob=PROB, min_inliers=MIN_INL, max_its_cap=CAP)
    args.update(kw)
    try:
        ss.sim3_solver(c["rig"], c["kf1"], c["pts1"], c["kf2s"], c["pts2s"], args.pop("matches12"), c["ok1"], c["ok2s"],
                       c["first1"], c["first2s"], c["sigma2"], c["samples"], **args)
    except mcs_amd.McsError as e:
        return e.code
    return mcs_amd.MCS_OK


def test_host_entry_without_a_device(built):
    import mcs_amd
    if mcs_amd.device_count() > 0:
        pytest.skip("a device is visible")
    assert _host_call() == mcs_amd.MCS_ERR_NO_DEVICE


@pytest.mark.parametrize("kw", [dict(n_iterations=0), dict(n_iterations=CAP + 1), dict(min_inliers=0), dict(prob=1.0),
                                dict(prob=0.0), dict(flags=8)], ids=lambda k: "%s_%s" % next(iter(k.items())))
def test_argument_errors_come_before_any_device_use(built, kw):
    import mcs_amd
    assert _host_call(**kw) == mcs_amd.MCS_ERR_ARG, mcs_amd.lib().mcs_last_error()
