"""Generate tests/golden/sim3solver_ref.npz: what the reference TEXT of cSim3Solver gives, evaluated
by tests/golden/cxx_eval.py (safe_exec, no builtins).  No reference source is stored: the fixture
holds numbers only.

Translated from /root/reference:
  cSim3Solver::cSim3Solver                  src/cSim3Solver.cpp:44-137
  cSim3Solver::SetRansacParameters          src/cSim3Solver.cpp:139-165
  cSim3Solver::iterate                      src/cSim3Solver.cpp:167-254
  cSim3Solver::centroid, computeT           src/cSim3Solver.cpp:264-371
  cSim3Solver::CheckInliers                 src/cSim3Solver.cpp:374-415
  the member declarations of the class      include/cSim3Solver.h (mvnMaxError1 / 2 are
      std::vector<size_t>, so push_back(9.210 * sigma2) at :106-107 truncates)
Three parts:
  max_its   mRansacMaxIts for every N of N_LIST under the call site's (0.98, 15, 300)
            (src/cLoopClosing.cpp:313) and the constructor's defaults (0.99, 6, 300);
  ctor<seed>_*  the constructor on the scripted map of gen_sim3_ref.py / gen_fuse_ref.py (World): every
            skip rule, points observed first at another keypoint than their slot; the rows it builds;
  it_<case>_<t>_*  SetRansacParameters(0.98, 15, 300) and six visits of iterate(50) on the candidates of
            tests/test_sim3solver_ref.py's cases with their scripted draws (see run_iterate).
The constructs the translator lacks and the stand-ins are listed above load_iterate; cxx_eval.py and
the other generators are not edited.

    python tests/golden/gen_sim3solver_ref.py [--ref /root/reference] [--out tests/golden/sim3solver_ref.npz]
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "multicol-slam-annotation_amd"))
import cxx_rt as rt  # noqa: E402
import gen_matcher_ref as gm  # noqa: E402
from cxx_eval import INT, VOID, ClassSpec, Cls, build_env, class_body, parse_members, translate_function  # noqa: E402
from safe_exec import safe_exec  # noqa: E402

N_LIST = list(range(15, 201)) + [250, 300, 400, 1000, 6000]
PARAMS = [(0.98, 15, 300), (0.99, 6, 300)]
VECTORS = ("mvnIndices1", "mvnMaxError1", "mvnMaxError2", "mvAllIndices", "camIdx1", "camIdx2")


def load(ref):
    ctx, _, _, macros, _, _ = gm.setup(ref)
    cpp = open(os.path.join(ref, "src", "cSim3Solver.cpp"), encoding="latin-1").read()
    hdr = open(os.path.join(ref, "include", "cSim3Solver.h"), encoding="latin-1").read()
    sv = ClassSpec("cSim3Solver", ctor="Solver_")
    ctx.add_class(sv)
    sv.fields = parse_members(ctx, class_body(hdr, "cSim3Solver"))
    params, _, body = gm.find_fn(cpp, r"void cSim3Solver::SetRansacParameters\(")
    src = translate_function(ctx, "f_SetRansacParameters", params, body, this_cls=sv, ret=VOID, macros=macros)
    G = safe_exec(src, build_env(ctx, rt, {"Matx33d_": lambda: None, "Matx44d_": lambda: None}), "<ref:cSim3Solver.cpp>")
    return G, sv, body.count(";")


# ------------------------------------------------------------------------------ the constructor
CTOR_SEEDS = (901, 902)


def ctor_inputs(seed):
    """Two keyframes of the Lafida rig and a scripted map: point m < n1 sits in KF1's slot m, point
    n1 + k in KF2's slot k, except that some slots hold the point of a LOWER slot (the point then
    observes its keyframe at two keypoints and GetIndexInKeyFrame()[0] is the lower one), some are
    NULL, some points are bad (a bad point observes nothing), and some good points do not observe
    their keyframe at all (first index -1).  vpMatched12 covers every skip rule."""
    from tests.test_fuse_ref import make_rig, make_target
    rng = np.random.default_rng(seed)
    rig = make_rig(3)
    kfs = [make_target(rig, rng, 30, 32, False) for _ in range(2)]
    n = [len(k["kp_xy"]) for k in kfs]
    pos = rng.normal(0, 3.0, (n[0] + n[1], 3))
    slots, has, bad, unobs = [], [], [], []
    for t in range(2):
        base = 0 if t == 0 else n[0]
        sl = base + np.arange(n[t])
        for b in rng.choice(np.arange(4, n[t]), n[t] // 5, replace=False):      # a second observation
            sl[b] = base + int(rng.integers(0, b))
        h = rng.random(n[t]) < 0.9
        sl = np.where(h, sl, -1).astype(np.int32)
        slots.append(sl)
        has.append(h)
        bad.append(rng.random(n[0] + n[1]) < 0.08)
        unobs.append(rng.random(n[0] + n[1]) < 0.08)
    mp_bad = (bad[0] | bad[1]).astype(np.uint8)
    m12 = np.full(n[0], -1, np.int32)
    for i in rng.choice(n[0], (2 * n[0]) // 3, replace=False):
        m12[i] = int(rng.choice(np.flatnonzero(has[1])))
    return rig, kfs, pos, slots, mp_bad, unobs[0] & (mp_bad == 0), m12


def run_ctor(G, R, Matx, gf, gs, seed, out):
    rig, kfs, pos, slots, mp_bad, unobs, m12 = ctor_inputs(seed)
    n1, n2 = len(kfs[0]["kp_xy"]), len(kfs[1]["kp_xy"])
    N = n1 + n2
    sigma2 = np.asarray(rig["scale"], np.float64) ** 2
    q = dict(pos=pos, dist=np.ones((N, 2)), desc=np.zeros((N, 32), np.uint8), mask=None)
    obs = [np.zeros(N, np.uint8), np.zeros(N, np.uint8)]
    for t in range(2):
        obs[t][slots[t][slots[t] >= 0]] = 1
        obs[t][(mp_bad != 0) | unobs] = 0
    W = gf.World(G, R, Matx, rig, kfs, q, np.arange(N, dtype=np.int32), mp_bad, slots, obs, q["desc"], 32, False)
    for t, kf in enumerate(W.kfs):
        kf.f["mMutexPose"] = None
        kf.f["GetMapPointMatches"] = lambda kf=kf: G["f_kf_GetMapPointMatches"](kf)
        kf.f["GetKeyPoint"] = lambda i, kf=kf: kf["mvKeys"].v[i]
        kf.f["GetSigma2"] = lambda lv: float(sigma2[lv])
        w4 = kf["camSystem"]["WorldToCamHom_fast"]
        # the Vec3d overload (src/cam_system_omni.cpp:114-133) is the Vec4d one on (pt3, 1.0)
        kf["camSystem"].f["WorldToCamHom_fast"] = lambda c, p3, uv, w4=w4: w4(c, gf._vec(list(p3.v) + [1.0]), uv)
    for mp in W.mps:
        mp.f["GetIndexInKeyFrame"] = lambda pKF, mp=mp: G["f_mp_GetIndexInKeyFrame"](mp, pKF)
    vp12 = rt.Vector(lambda: None, [W.mp_ptr[int(slots[1][k])] if k >= 0 else None for k in m12])
    S = G["Solver_"]()
    G["f_s3s_ctor"](S, W.kf_ptr[0], W.kf_ptr[1], vp12, W.kfs[0]["camSystem"])
    first = []
    for t in range(2):
        f = np.full(len(slots[t]), -1, np.int32)
        for i, m in enumerate(slots[t]):
            if m >= 0:
                f[i] = int(W.mps[int(m)]["GetIndexInKeyFrame"](W.kf_ptr[t]).v[0])
        first.append(f)
    p = "ctor%d_" % seed
    for t, tag in enumerate(("k1_", "k2_")):
        for k in ("kp_xy", "kp_octave", "kp_cam", "m_t"):
            out[p + tag + k] = kfs[t][k]
        out[p + tag + "slots"], out[p + tag + "first"] = slots[t], first[t]
    out[p + "pos"], out[p + "mp_bad"], out[p + "matches12"], out[p + "sigma2"] = pos, mp_bad, m12, sigma2
    vec = lambda name, w: np.array([list(x.v) for x in S[name].v], np.float64).reshape(-1, w)  # noqa: E731
    ints = lambda name: np.array(list(S[name].v), np.int64)  # noqa: E731
    out[p + "N"], out[p + "max_its"] = np.int32(S["N"]), np.int32(S["mRansacMaxIts"])
    out[p + "idx1"], out[p + "cam1"], out[p + "cam2"] = ints("mvnIndices1"), ints("camIdx1"), ints("camIdx2")
    out[p + "maxerr1"], out[p + "maxerr2"], out[p + "all"] = ints("mvnMaxError1"), ints("mvnMaxError2"), ints("mvAllIndices")
    out[p + "X1"], out[p + "X2"], out[p + "p1"], out[p + "p2"] = vec("mvX3Dc1", 3), vec("mvX3Dc2", 3), vec("mvP1im1", 2), vec("mvP2im2", 2)
    return int(S["N"]), int((m12 >= 0).sum())


def load_ctor(ref):
    """gen_sim3_ref.load (Fuse + SearchBySim3 translations and stand-ins) plus the solver's
    constructor and SetRansacParameters."""
    import cxx_eval
    import gen_fuse_ref as gf
    import gen_sim3_ref as gs
    from cxx_eval import DOUBLE, Fn
    base = gs.translate_all

    def translate_all(ref_):
        ctx, srcs, n_stmt = base(ref_)
        cpp = open(os.path.join(ref_, "src", "cSim3Solver.cpp"), encoding="latin-1").read()
        hdr = open(os.path.join(ref_, "include", "cSim3Solver.h"), encoding="latin-1").read()
        sv = ClassSpec("cSim3Solver", ctor="Solver_")
        ctx.add_class(sv)
        sv.fields = parse_members(ctx, class_body(hdr, "cSim3Solver"))
        sv.methods["SetRansacParameters"] = Fn("f_s3s_setp", [gm.val(DOUBLE), gm.val(INT), gm.val(INT)], VOID,
                                                defaults=["0.99", "6", "300"])     # include/cSim3Solver.h:46-48
        ctx.classes["cMultiKeyFrame"].methods["GetSigma2"] = gm._sig([gm.val(INT)], DOUBLE)
        macros = gm.setup(ref_)[3]
        for pyname, pat, ctor in (("f_s3s_ctor", r"cSim3Solver::cSim3Solver\(", True),
                                  ("f_s3s_setp", r"void cSim3Solver::SetRansacParameters\(", False)):
            params, init, body = gm.find_fn(cpp, pat)
            n_stmt += body.count(";")
            with gs.swapped(cxx_eval, "FuncTranslator", gs.Sim3Translator):
                srcs.append(translate_function(ctx, pyname, params, body, this_cls=sv, ret=VOID, macros=macros,
                                               init_text=init if ctor else None))
        return ctx, srcs, n_stmt
    with gs.swapped(gs, "translate_all", translate_all):
        G, R, Matx = gs.load(ref)
    return G, R, Matx, gf, gs


# ------------------------------------------------------------------------------ iterate
# iterate (:167-254), centroid and computeT (:264-371) and CheckInliers (:374-415) use constructs the
# translator lacks; as gen_sim3_ref.py does, they are added here and cxx_eval.py is not edited:
#   cv::Matx33d / Matx44d / Matx<double,4,1> / cv::Mat become ONE mutable matrix class (MX) with
#   element access M(i, j) as an lvalue, so `P3Dc1i(0, i) = ...` and `Pr(0, i) = ...` translate;
#   `C /= 3.0` on a cv::Vec (multiplies by 1. / alpha, as OpenCV's operator does);
#   `N = (cv::Mat_<double>(4, 4) << a, b, ...)`; unary minus on a Matx; .t(), .dot(), .row(),
#   .colRange(), .copyTo(), .ptr<double>().
# Stand-ins: std::random_device / std::mt19937 / std::uniform_int_distribution -> dis(gen) returns the
# scripted draws (and checks the range is 0 .. N-1 every time); cv::eigen -> numpy.linalg.eigh sorted
# descending, eigenvectors in rows; cv::Rodrigues, cv::pow(., 2, .), Matx::dot, cv::norm, the Matx /
# Vec arithmetic (products accumulate s = 0; s += a_k * b_k in order), cConverter::invMat / Rt2Hom /
# toVec4d, cMultiCamSys_::Get_M_c and WorldToImg (RefMath's, which refmath.npz pins) as restatements.
MATS = ("Matx33d", "Matx44d", "Matx", "Mat")


class MX(rt.Mat):
    """A cv::Matx / cv::Mat of doubles with value semantics."""
    __slots__ = ("a",)

    def __init__(self, rows=0, cols=0, typ=0):
        self.a = np.zeros((int(rows), int(cols)))

    def __getitem__(self, k):
        if k == "rows":
            return self.a.shape[0]
        if k == "cols":
            return self.a.shape[1]
        return float(self.a[k])

    def __setitem__(self, k, v):
        self.a[k] = v

    def copy(self):
        m = MX()
        m.a = self.a.copy()
        return m

    def assign(self, o):
        self.a = o.a.copy()


class UVector(rt.Vector):
    """std::vector as the text's sampling loop uses it (:202-222): the distribution stays 0 .. N-1
    while pop_back shrinks the vector, so operator[] reads at or past size().  That is out of range in
    the text; an unchecked std::vector returns what the storage still holds.  pop_back here lowers
    size() and keeps the storage; operator[] reaches the storage; back() is the element at size() - 1."""
    __slots__ = ("n",)

    def __init__(self, fac, items=None):
        rt.Vector.__init__(self, fac, items)
        self.n = len(self.v)

    def copy(self):
        return UVector(self.fac, [rt.cp(x) for x in self.v[:self.n]])

    def assign(self, o):
        self.v = [rt.cp(x) for x in o.v[:o.m_size()]]
        self.n = len(self.v)

    def m_size(self):
        return self.n

    def m_empty(self):
        return self.n == 0

    def m_resize(self, n, val=None):
        del self.v[self.n:]
        rt.Vector.m_resize(self, n, val)
        self.n = len(self.v)

    def m_push_back(self, x):
        del self.v[self.n:]
        rt.Vector.m_push_back(self, x)
        self.n = len(self.v)

    def m_pop_back(self):
        self.n -= 1

    def m_back(self):
        return self.v[self.n - 1]


def _mx(a):
    m = MX()
    m.a = np.array(a, np.float64)
    return m


def iterate_env(R, cams_d, rig, draws_box):
    """The stand-ins of the iterate group."""
    import math
    from tests.test_fuse_ref import _inv_mat
    vec = lambda xs: rt.Vector(lambda: 0.0, [float(x) for x in xs])  # noqa: E731

    def col(b):
        return np.array(b.v, np.float64).reshape(-1, 1) if isinstance(b, rt.Vector) else b.a

    def matmul(A, B):
        a, b = A.a, col(B)
        out = np.zeros((a.shape[0], b.shape[1]))
        for i in range(a.shape[0]):
            for j in range(b.shape[1]):
                sm = 0.0
                for k in range(a.shape[1]):
                    sm += float(a[i, k]) * float(b[k, j])
                out[i, j] = sm
        return _mx(out)

    def scale(alpha, X):
        if isinstance(X, rt.Vector):
            return vec([x * alpha for x in X.v])
        return _mx(X.a * alpha)

    def dot(a, b):
        xa = a.v if isinstance(a, rt.Vector) else list(np.ravel(a.a))
        xb = b.v if isinstance(b, rt.Vector) else list(np.ravel(b.a))
        sm = 0.0
        for x, y in zip(xa, xb):
            sm += float(x) * float(y)
        return sm

    def norm(m):
        sm = 0.0
        for x in np.ravel(m.a):
            sm += float(x) * float(x)
        return math.sqrt(sm)

    def eigen(N, ev, evec):
        w, v = np.linalg.eigh(N.a)
        order = np.argsort(-w, kind="stable")
        ev.a, evec.a = w[order].reshape(-1, 1).copy(), v[:, order].T.copy()

    def rodrigues(v, Rm):
        r = np.ravel(v.a)
        th = math.sqrt(float(r @ r))
        if th < np.finfo(np.float64).eps:
            Rm.a = np.eye(3)
            return
        x, y, z = r / th
        c, sn = math.cos(th), math.sin(th)
        K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
        Rm.a = c * np.eye(3) + (1 - c) * np.outer([x, y, z], [x, y, z]) + sn * K

    def rt2hom(Rm, t):
        out = np.eye(4)
        out[:3, :3], out[:3, 3] = Rm.a, t.v
        return _mx(out)

    class Dis:
        def __init__(self, lo, hi):
            assert lo == 0 and hi == draws_box["N"] - 1, (lo, hi)

        def __getitem__(self, k):
            return lambda gen: int(draws_box["draws"].pop(0))

    class Rd:
        def __getitem__(self, k):
            return lambda: 0

    def mat_ctor(*a):
        return MX(a[0], a[1]) if len(a) >= 2 else MX()

    def pow2(P, p, out=None):                # cv::pow(Matx, 2, Matx); std::pow on two numbers
        if out is None:
            return math.pow(P, p)
        assert p == 2
        out.a = P.a * P.a

    def copy_to(src, dst):
        dst.a = src.a.copy()
    with np.errstate(all="ignore"):
        pass
    return {
        "MX_Matx33d": lambda: MX(3, 3), "MX_Matx44d": lambda: MX(4, 4), "MX_Matx": lambda: MX(4, 1), "MX_Mat": mat_ctor,
        "C_random_device": Rd, "C_mt19937": lambda seed: None, "C_uniform_int_distribution": Dis, "C_Mat_": None,
        "c_CV_64FC1": 6, "s_matmul": matmul, "s_matvec": lambda A, x: vec(np.ravel(matmul(A, x).a)),
        "s_scale": scale, "s_scale_r": lambda X, alpha: scale(alpha, X), "s_div": lambda X, d: _mx(X.a * (1.0 / d)),
        "s_sub": lambda a, b: vec([x - y for x, y in zip(a.v, b.v)]), "s_add": lambda a, b: vec([x + y for x, y in zip(a.v, b.v)]),
        "s_vec_div": lambda v, alpha: vec([x * (1.0 / alpha) for x in v.v]), "s_t": lambda A: _mx(A.a.T), "s_dot": dot,
        "s_row": lambda A, r: _mx(A.a[r:r + 1]), "s_colRange": lambda A, c0, c1: _mx(A.a[:, c0:c1]), "s_copyTo": copy_to,
        "s_rowptr": lambda A, r: [float(x) for x in A.a[r]], "s_mat_init": lambda r, c, xs: _mx(np.array(xs).reshape(r, c)),
        "s_Matx33d__zeros": lambda: MX(3, 3), "s_Matx33d__eye": lambda: _mx(np.eye(3)), "s_Matx44d__eye": lambda: _mx(np.eye(4)),
        "s_cConverter__toVec4d": lambda v: vec(list(v.v) + [1.0]), "s_cConverter__invMat": lambda M: _mx(_inv_mat(M.a)),
        "s_cConverter__Rt2Hom": rt2hom, "s_eigen": eigen, "s_cv__eigen": eigen, "s_Rodrigues": rodrigues,
        "s_cv__Rodrigues": rodrigues, "s_pow": pow2, "s_cv__pow": pow2, "s_norm": norm, "s_cv__norm": norm,
        "_atan2": math.atan2, "_Vector": UVector,
    }


def load_iterate(ref):
    import re
    import cxx_eval
    from cxx_eval import BOOL, DOUBLE, E, Fn, PtrT
    M33, M44, MAT = Cls("Matx33d"), Cls("Matx44d"), Cls("Mat")

    class IterTranslator(cxx_eval.FuncTranslator):
        def conv(self, e, to):
            names = MATS + ("Vec", "MatExpr")
            if isinstance(to, Cls) and isinstance(e.ty, Cls) and to.name in names and e.ty.name in names:
                return e.code
            return super().conv(e, to)

        def ex_un(self, n):
            if n[1] == "-":
                e = self.ex(n[2])
                if isinstance(e.ty, Cls) and e.ty.name in MATS:
                    return E("s_scale(-1.0, %s)" % e.code, e.ty, obj=True)
            return super().ex_un(n)

        def method_call(self, code, oty, mname, targs, args):
            if isinstance(oty, Cls) and oty.name in MATS:
                es = [self.ex(a) for a in args]
                if mname == "()":
                    k = "(%s)" % ", ".join([self.conv(x, INT) for x in es] + (["0"] if len(es) == 1 else []))
                    return E("%s[%s]" % (code, k), DOUBLE, ("sub", code, k))
                one = {"t": ("s_t(%s)", oty), "row": ("s_row(%s, %s)", MAT), "colRange": ("s_colRange(%s, %s, %s)", MAT)}
                if mname in one:
                    fmt, ty = one[mname]
                    return E(fmt % tuple([code] + [self.conv(x, INT) for x in es]), ty, obj=True)
                if mname == "dot":
                    return E("s_dot(%s, %s)" % (code, es[0].code), DOUBLE)
                if mname == "copyTo":
                    return E("s_copyTo(%s, %s)" % (code, es[0].code), VOID)
                if mname == "type":
                    return E("0", INT)
                if mname == "ptr":
                    return E("s_rowptr(%s, %s)" % (code, self.conv(es[0], INT)), PtrT(DOUBLE))
            if isinstance(oty, Cls) and oty.name == "Vec" and mname == "dot":
                return E("s_dot(%s, %s)" % (code, self.ex(args[0]).code), DOUBLE)
            return super().method_call(code, oty, mname, targs, args)

        def assign_stmt(self, e):
            _, op, lhs_n, rhs_n = e
            r = rhs_n
            while r[0] == "paren":
                r = r[1]
            if op == "=" and r[0] == "comma" and r[1][0][0] == "bin" and r[1][0][1] == "<<":
                first = r[1][0]                  # (cv::Mat_<double>(rows, cols) << v0), v1, ...
                dims = [self.conv(self.ex(a), INT) for a in first[2][2]]
                vals = [self.conv(self.ex(x), DOUBLE) for x in [first[3]] + list(r[1][1:])]
                return ["_assign(%s, s_mat_init(%s, %s, [%s]))" % (self.ex(lhs_n).code, dims[0], dims[1], ", ".join(vals))]
            if op == "/=":
                lhs = self.ex(lhs_n)
                if isinstance(lhs.ty, Cls) and lhs.ty.name == "Vec":
                    return ["_assign(%s, s_vec_div(%s, %s))" % (lhs.code, lhs.code, self.conv(self.ex(rhs_n), DOUBLE))]
            return super().assign_stmt(e)

    saved = set(cxx_eval.VALUE_CLASSES)
    try:
        ctx, _, _, macros, _, _ = gm.setup(ref)
        for n in MATS:                          # mutable objects here, not immutable values
            cxx_eval.VALUE_CLASSES.discard(n)
            ctx.add_class(ClassSpec(n, {"cols": INT, "rows": INT}, ctor="MX_" + n))
            ctx.classes[n].runtime_ctor = {"Matx33d": lambda *a: MX(3, 3), "Matx44d": lambda *a: MX(4, 4),
                                           "Matx": lambda *a: MX(4, 1), "Mat": lambda *a: MX(*a[:2])}[n]
        for n in ("random_device", "mt19937", "uniform_int_distribution", "Mat_"):
            ctx.add_class(ClassSpec(n, ctor="C_" + n))
        ctx.classes["random_device"].methods["()"] = gm._sig([], INT)
        ctx.classes["uniform_int_distribution"].methods["()"] = gm._sig([gm.m_ref(Cls("mt19937"))], INT)
        ctx.classes["cMultiCamSys_"].methods["Get_M_c"] = gm._sig([gm.val(INT)], M44)
        ctx.classes["cCamModelGeneral_"].methods["WorldToImg"] = gm._sig([gm.c_ref(DOUBLE)] * 3 + [gm.m_ref(DOUBLE)] * 2, VOID)
        cpp = open(os.path.join(ref, "src", "cSim3Solver.cpp"), encoding="latin-1").read()
        hdr = open(os.path.join(ref, "include", "cSim3Solver.h"), encoding="latin-1").read()
        sv = ClassSpec("cSim3Solver", ctor="Solver_")
        ctx.add_class(sv)
        sv.fields = parse_members(ctx, class_body(hdr, "cSim3Solver"))
        sv.methods["CheckInliers"] = Fn("f_CheckInliers", [], VOID)
        sv.methods["centroid"] = Fn("f_centroid", [gm.m_ref(M33), gm.m_ref(M33), gm.m_ref(gm.VEC3)], VOID)
        sv.methods["computeT"] = Fn("f_computeT", [gm.m_ref(M33), gm.m_ref(M33)], VOID)
        first, second = (lambda a, b: a), (lambda a, b: b)
        for A in MATS:
            for B in MATS:
                ctx.binops[(A, "*", B)] = ("s_matmul", second if B == "Matx" else first)
            ctx.binops[(A, "*", "Vec")] = ("s_matvec", second)
            ctx.binops[("arith", "*", A)] = ("s_scale", second)
            ctx.binops[(A, "*", "arith")] = ("s_scale_r", first)
            ctx.binops[(A, "/", "arith")] = ("s_div", first)
        ctx.binops.update({("arith", "*", "Vec"): ("s_scale", second), ("Vec", "-", "Vec"): ("s_sub", first),
                           ("Vec", "+", "Vec"): ("s_add", first)})
        for name, ty in [("Matx33d::zeros", M33), ("Matx33d::eye", M33), ("Matx44d::eye", M44), ("cConverter::toVec4d", gm.VEC4),
                         ("cConverter::invMat", M44), ("cConverter::Rt2Hom", M44), ("cv::eigen", VOID), ("eigen", VOID),
                         ("cv::Rodrigues", VOID), ("Rodrigues", VOID), ("cv::pow", VOID), ("pow", lambda ts: VOID if isinstance(ts[0], Cls) else DOUBLE), ("norm", DOUBLE),
                         ("cv::norm", DOUBLE)]:
            ctx.funcs[name] = Fn("s_" + re.sub(r"\W", "_", name), None, ty)
        ctx.consts["CV_64FC1"] = ("c_CV_64FC1", INT)
        srcs, n_stmt = [], 0
        with __import__("gen_sim3_ref").swapped(cxx_eval, "FuncTranslator", IterTranslator):
            for name, pat, ret in [("f_iterate", r"bool cSim3Solver::iterate\(", BOOL), ("f_centroid", r"void cSim3Solver::centroid\(", VOID),
                                   ("f_computeT", r"void cSim3Solver::computeT\(", VOID),
                                   ("f_CheckInliers", r"void cSim3Solver::CheckInliers\(", VOID),
                                   ("f_SetRansacParameters", r"void cSim3Solver::SetRansacParameters\(", VOID)]:
                params, _, body = gm.find_fn(cpp, pat)
                n_stmt += body.count(";")
                srcs.append(translate_function(ctx, name, params, body, this_cls=sv, ret=ret, macros=macros))
        return ctx, srcs, n_stmt
    finally:
        cxx_eval.VALUE_CLASSES.clear()
        cxx_eval.VALUE_CLASSES.update(saved)


ITER_CASES = ("t3_mixed", "t3_small")
N_VISITS = 6                 # visits of 50 per candidate, as ComputeSim3 makes them (src/cLoopClosing.cpp:343)


def run_iterate(ref, out):
    """The solver's members are filled from the constructor's rows (which the ctor scenarios pin),
    then SetRansacParameters(0.98, 15, 300) and N_VISITS x iterate(50) run from the text with the
    scripted draws of tests/test_sim3solver_ref.py's cases.  Recorded per evaluated iteration: the
    3 x 3 point sets handed to computeT (what the draws selected), s, R, t, mvbInliersi and
    mnInliersi; per visit: the return value, bNoMore, nInliers, vbInliers, result, mnIterations,
    mnBestInliers and the mBest* members."""
    from tests.test_sim3solver_ref import CAP, MIN_INL, PROB, get_case
    ctx, srcs, n_stmt = load_iterate(ref)
    R = gm.make_refmath(ref)[0]
    box = {}
    rig = get_case(ITER_CASES[0])["rig"]
    cams_d = [dict(c, p=c["a"], invp=c["pol"]) for c in rig["cams"]]
    env = build_env(ctx, rt, iterate_env(R, cams_d, rig, box))
    G = safe_exec("\n".join(srcs), env, "<ref:cSim3Solver.cpp iterate>")
    vec = lambda xs: rt.Vector(lambda: 0.0, [float(x) for x in xs])  # noqa: E731
    ivec = lambda xs: rt.Vector(lambda: 0, [int(x) for x in xs])  # noqa: E731

    def cam_obj(c):
        def w2i(x, y, z, u, v):
            u[0], v[0] = R.world_to_img(cams_d[c], x, y, z)
        return gm.Obj(WorldToImg=w2i)
    cam_objs = [cam_obj(c) for c in range(len(cams_d))]
    Mc = [_mx(np.asarray(rig["m_c"][c], np.float64).reshape(4, 4)) for c in range(len(cams_d))]
    camsys = rt.Ptr(obj=gm.Obj(Get_M_c=lambda c: Mc[c].copy(), GetCamModelObj=lambda c: cam_objs[c]))
    rec = {}
    compute_t, check = G["f_computeT"], G["f_CheckInliers"]

    def compute_rec(S, P1, P2):
        compute_t(S, P1, P2)
        rec["P1"].append(P1.a.copy())
        rec["P2"].append(P2.a.copy())
        rec["srt"].append(np.concatenate([[S["ms12i"]], np.ravel(S["mR12i"].a), S["mt12i"].v]))

    def check_rec(S):
        check(S)
        rec["inl"].append(np.array([bool(b) for b in S["mvbInliersi"].v], np.uint8))
        rec["cnt"].append(int(S["mnInliersi"]))
    G["f_computeT"], G["f_CheckInliers"] = compute_rec, check_rec
    for name in ITER_CASES:
        case = get_case(name)
        n1 = len(case["kf1"]["kp_xy"])
        for t, rows in enumerate(case["rows"]):
            N = rows["n"]
            S = G["Solver_"]()
            S["mN1"], S["camSysLocal"] = n1, camsys
            S["mvpMapPoints1"] = rt.Vector(lambda: None, [None] * N)
            S["mvX3Dc1"] = rt.Vector(lambda: vec([0, 0, 0]), [vec(x) for x in rows["X1"]])
            S["mvX3Dc2"] = rt.Vector(lambda: vec([0, 0, 0]), [vec(x) for x in rows["X2"]])
            S["mvP1im1"] = rt.Vector(lambda: vec([0, 0]), [vec(x) for x in rows["p1"]])
            S["mvP2im2"] = rt.Vector(lambda: vec([0, 0]), [vec(x) for x in rows["p2"]])
            S["camIdx1"], S["camIdx2"], S["mvnIndices1"] = ivec(rows["cam1"]), ivec(rows["cam2"]), ivec(rows["idx1"])
            S["mvnMaxError1"], S["mvnMaxError2"] = ivec(rows["maxerr1"]), ivec(rows["maxerr2"])
            S["mvAllIndices"] = ivec(range(N))
            S["mnIterations"], S["mnBestInliers"] = 0, 0                     # the constructor's initialisers (:48-49)
            try:
                G["f_SetRansacParameters"](S, PROB, MIN_INL, CAP)
            except ValueError:
                # N < minInliers: log(1 - pow(epsilon, 3)) of a negative number; the text converts a NaN
                # to int there.  N and mRansacMinInliers are set by then, and iterate returns at :177
                # before mRansacMaxIts is read.
                assert N < MIN_INL and S["N"] == N and S["mRansacMinInliers"] == MIN_INL
            for k in ("P1", "P2", "srt", "inl", "cnt"):
                rec[k] = []
            box["N"], box["draws"] = N, [int(x) for x in np.ravel(case["draws"][t])]
            visits, inl_out, best = [], [], []
            for _ in range(N_VISITS):
                no_more, n_inl = [False], [0]
                vb, res = rt.Vector(lambda: False), MX(4, 4)
                ok = G["f_iterate"](S, 50, no_more, vb, n_inl, res)
                visits.append([int(ok), int(no_more[0]), int(n_inl[0]), int(S["mnIterations"]), int(S["mnBestInliers"])])
                inl_out.append(np.array([bool(b) for b in vb.v], np.uint8))
                best.append(np.concatenate([[S["mBestScale"]], np.ravel(S["mBestRotation"].a), S["mBestTranslation"].v,
                                            np.ravel(S["mBestT12"].a), np.ravel(res.a)]))
            p = "it_%s_%d_" % (name, t)
            out[p + "N"], out[p + "max_its"] = np.int32(N), np.int32(S["mRansacMaxIts"] if N >= MIN_INL else 0)
            out[p + "visits"] = np.array(visits, np.int32).reshape(N_VISITS, 5)
            out[p + "vbInliers"] = np.array(inl_out, np.uint8).reshape(N_VISITS, n1)
            out[p + "best"] = np.array(best, np.float64).reshape(N_VISITS, 45)
            out[p + "P1"] = np.array(rec["P1"], np.float64).reshape(-1, 3, 3)
            out[p + "P2"] = np.array(rec["P2"], np.float64).reshape(-1, 3, 3)
            out[p + "srt"] = np.array(rec["srt"], np.float64).reshape(-1, 13)
            out[p + "inl"] = np.array(rec["inl"], np.uint8).reshape(-1, N)
            out[p + "cnt"] = np.array(rec["cnt"], np.int32)
            print("iterate", name, t, "N", N, "evaluated", len(rec["cnt"]), "visits", visits)
    return n_stmt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(HERE, "sim3solver_ref.npz"))
    a = ap.parse_args()
    G, sv, n_stmt = load(a.ref)
    max_its = np.zeros((len(PARAMS), len(N_LIST)), np.int32)
    for p, (prob, mn, cap) in enumerate(PARAMS):
        for j, N in enumerate(N_LIST):
            if N < mn:
                max_its[p, j] = -1
                continue
            S = G["Solver_"]()
            S["mvpMapPoints1"] = rt.Vector(lambda: None, [None] * N)
            S["mnIterations"] = 7
            G["f_SetRansacParameters"](S, prob, mn, cap)
            assert S["mnIterations"] == 0 and S["N"] == N and S["mvbInliersi"]["size"]() == N
            max_its[p, j] = S["mRansacMaxIts"]
    out = {}
    Gc, R, Matx, gf, gs = load_ctor(a.ref)
    for seed in CTOR_SEEDS:
        print("ctor", seed, "N, matches:", run_ctor(Gc, R, Matx, gf, gs, seed, out))
    n_iter = run_iterate(a.ref, out)
    out["n_statements_iterate"] = np.int32(n_iter)
    out["iterate_cases"] = np.array(ITER_CASES)
    integral = np.array([sv.fields[k] == Cls("vector", (INT,)) for k in VECTORS], np.uint8)
    np.savez_compressed(a.out, n_statements=np.int32(n_stmt), n_list=np.array(N_LIST, np.int32),
                        params=np.array(PARAMS, np.float64), max_its=max_its, vectors=np.array(VECTORS),
                        vector_is_integral=integral, ctor_seeds=np.array(CTOR_SEEDS, np.int32), **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes; max_its at N = 50:", max_its[0][N_LIST.index(50)])


if __name__ == "__main__":
    main()
