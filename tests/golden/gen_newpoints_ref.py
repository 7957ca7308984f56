"""Generate tests/golden/newpoints_ref.npz: the per-match loop of cLocalMapping::CreateNewMapPoints,
evaluated from the reference TEXT on scripted keyframes of the Lafida rig (no reference source is
stored: the fixture holds numbers only).

Translated from /root/reference by tests/golden/cxx_eval.py (safe_exec, no builtins), on top of what
tests/golden/gen_fuse_ref.py and gen_sim3_ref.py translate (cMultiCamSys_::WorldToCamHom_fast among
them) and through tests/golden/gen_refmath.py (RefMath: cConverter::invMat,
cCamModelGeneral_::WorldToImg):
  the loop `for (size_t ikp = 0, ...` of cLocalMapping::CreateNewMapPoints up to the scale test,
      src/cLocalMapping.cpp:272-364, as it stands in the function body (LOOP_PARAMS below names the
      function's locals and file-scope constants the loop reads: they become parameters)
  triangulate_point                                          src/misc.cpp:26-51
Stand-ins, all in this file (cxx_eval.py, cxx_rt.py and the other generators are not edited):
  * the tail `cMapPoint* pMP = new cMapPoint(...)` ... `++testCnt` (:365-381) is replaced by one call
    of a recorder, rec_new(x3D, idx1, idx2): the admit step is pinned by mapside_ref.npz;
  * cv::Matx22d is a mutable 2 x 2 (element access A(i, j) as an lvalue) whose inv() is OpenCV's
    Matx_FastInvOp<_Tp, 2, 2> restated: d = 1 / det, then the adjugate times d, a zero matrix when
    det == 0.  OpenCV is not part of the reference tree; the library and the NumPy restatement use
    the same form, and tests/test_newpoints_ref.py measures what the other form (dividing by det)
    would change;
  * Matx44d::get_minor<3, 3>(0, 0) copies the 3 x 3 block (the parser has no template member calls,
    so its template arguments are folded into the name before parsing); cv::Matx31d is carried as a Vec3d
    (dot, +, element access (i, 0)); Vec2d indexing b[i]; cv::saturate_cast<double>(float) widens (spelled as a plain
    function before parsing, for the same reason);
  * cv::Matx / cv::Vec arithmetic as gen_fuse_ref.py and gen_sim3_ref.py state it (products and dot
    accumulate s = 0; s += a_k * b_k in order; cv::norm = sqrt of the in-order sum of squares;
    alpha * v scales every element), Hom2R, Hom2T, Get_MtMc, Get_MtMc_inv, GetSigma2, pow, cv::sqrt.
Recorded per match, in vMatchedIndices order: idx1, idx2, the verdict (which `continue` ended the
iteration, 1 = the recorder was reached), cosParallax, ptRot(2) and the pixel error of both
WorldToCamHom_fast gates, dist1, dist2 and x3D in the world frame (NaN where the text does not get
there).  They are read off the calls the text makes (Vec::dot, cv::norm, triangulate_point,
WorldToImg, cv::sqrt, pow, the recorder), not recomputed.
The scenarios are tests/test_newpoints_ref.py's (make_scene): true points with sub-pixel noise and
the crafted rows of verdicts 2-7.  The generator refuses a scenario in which a crafted row's deciding
quantity lies within relative 1e-6 of its threshold, or in which a verdict 1-7 is missing overall.

    python tests/golden/gen_newpoints_ref.py [--ref /root/reference] [--out tests/golden/newpoints_ref.npz]
"""
import argparse
import math
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "multicol-slam-annotation_amd"))
import cxx_eval  # noqa: E402
import cxx_rt as rt  # noqa: E402
import gen_fuse_ref as gf  # noqa: E402
import gen_matcher_ref as gm  # noqa: E402
import gen_sim3_ref as gs  # noqa: E402
from cxx_eval import DOUBLE, INT, VOID, ClassSpec, Cls, E, Fn, build_env, translate_function  # noqa: E402

CRAFT_MARGIN = 1e-6
VEC3, M33, M44, M22, M31 = gm.VEC3, Cls("Matx33d"), Cls("Matx44d"), Cls("Matx22d"), Cls("Matx31d")
N_STMT = [0]
# the locals of CreateNewMapPoints (:227-269) and the file-scope constants (:39-43) the loop reads
LOOP_PARAMS = ("cMultiKeyFrame* mpCurrentMultiKeyFrame, std::vector<cMultiKeyFrame*>& vpNeighKFs, size_t i, "
               "cMultiKeyFrame* pKF2, std::vector<cv::Vec3d>& vMatchedKeysRays1, "
               "std::vector<cv::Vec3d>& vMatchedKeysRays2, std::vector<cv::KeyPoint>& vMatchedKeys1, "
               "std::vector<cv::KeyPoint>& vMatchedKeys2, std::vector<std::pair<size_t, size_t> >& vMatchedIndices, "
               "cv::Vec3d Ow1, cv::Vec3d Ow2, double baseline, double c_in_m1, double cosThresh, double pixelSize, "
               "double maxDIST")


class M22Obj:
    """cv::Matx22d with element access as an lvalue."""
    __slots__ = ("a",)

    def __init__(self):
        self.a = [[0.0, 0.0], [0.0, 0.0]]

    def __getitem__(self, k):
        return self.a[k[0]][k[1]]

    def __setitem__(self, k, v):
        self.a[k[0]][k[1]] = float(v)

    def copy(self):
        m = M22Obj()
        m.a = [list(r) for r in self.a]
        return m

    def assign(self, o):
        self.a = [list(r) for r in o.a]


def inv22(A):
    """Matx22d::inv() (OpenCV Matx_FastInvOp<_Tp, 2, 2>): d = 1 / det; the adjugate times d."""
    a = A.a
    d = a[0][0] * a[1][1] - a[0][1] * a[1][0]
    out = M22Obj()
    if d == 0:
        return out
    d = 1.0 / d
    out.a = [[a[1][1] * d, -a[0][1] * d], [-a[1][0] * d, a[0][0] * d]]
    return out


class NpTranslator(gs.Sim3Translator):
    """The translator plus the constructs of the loop and of triangulate_point it lacks (see the
    module docstring)."""
    VECS = ("Vec", "Matx31d")

    def conv(self, e, to):
        if isinstance(to, Cls) and isinstance(e.ty, Cls) and to.name in self.VECS and e.ty.name in self.VECS:
            return e.code
        return super().conv(e, to)

    def ex_index(self, n):
        base = self.ex(n[1])
        if isinstance(base.ty, Cls) and base.ty.name == "Vec":
            kc = self.conv(self.ex(n[2]), INT)
            return E("%s[%s]" % (base.code, kc), base.ty.args[0], ("sub", base.code, kc))
        return super().ex_index(n)

    def method_call(self, code, oty, mname, targs, args):
        name = oty.name if isinstance(oty, Cls) else None
        if name == "Matx22d" and mname == "()":
            k = "(%s)" % ", ".join(self.conv(self.ex(a), INT) for a in args)
            return E("%s[%s]" % (code, k), DOUBLE, ("sub", code, k))
        if name == "Matx22d" and mname == "inv":
            return E("s_inv22(%s)" % code, M22, obj=True)
        if name == "Matx31d" and mname == "()":
            es = [self.conv(self.ex(a), INT) for a in args]
            return E("%s[%s]" % (code, es[0]), DOUBLE, ("sub", code, es[0]))
        if name == "Matx31d" and mname == "dot":
            return E("s_vec_dot(%s, %s)" % (code, self.ex(args[0]).code), DOUBLE)
        if name == "Matx44d" and mname == "get_minor_3_3":
            es = [self.conv(self.ex(a), INT) for a in args]
            return E("s_get_minor(%s, %s, %s)" % (code, es[0], es[1]), M33, obj=True)
        return super().method_call(code, oty, mname, targs, args)


def loop_text(lm):
    """The text of the loop at :272 up to (not including) the `new cMapPoint` tail, closed again."""
    a = lm.index("for (size_t ikp = 0, iendkp = vMatchedKeysRays1.size()")
    b = lm.index("cMapPoint* pMP = new cMapPoint(x3D", a)
    # the parser has no template member calls: get_minor<3, 3>( is spelled get_minor_3_3( before parsing
    body = re.sub(r"get_minor\s*<\s*3\s*,\s*3\s*>\s*\(", "get_minor_3_3(", lm[a:b])
    body = re.sub(r"(?:cv::)?saturate_cast\s*<\s*double\s*>\s*\(", "saturate_cast_double(", body)   # likewise
    return body + "rec_new(x3D, idx1, idx2);\n}\n"


def translate_all(ref):
    ctx, srcs, n_stmt = gs.translate_all(ref)
    rd = lambda *p: open(os.path.join(ref, *p), encoding="latin-1").read()  # noqa: E731
    macros = gm.setup(ref)[3]
    cxx_eval.VALUE_CLASSES.discard("Matx22d")
    ctx.add_class(ClassSpec("Matx22d", ctor="M22_", runtime_ctor=M22Obj))
    ctx.add_class(ClassSpec("Matx31d", ctor="M31_", runtime_ctor=lambda: gf._vec([0.0] * 3)))
    ctx.classes["cMultiKeyFrame"].methods["GetSigma2"] = gm._sig([gm.val(INT)], DOUBLE)
    vec = lambda a, b: VEC3  # noqa: E731
    ctx.binops.update({("Matx22d", "*", "Vec"): ("s_m22_vec", lambda a, b: b), ("Matx31d", "+", "Vec"): ("s_vec_add", vec),
                       ("Matx31d", "+", "Matx31d"): ("s_vec_add", vec), ("Vec", "+", "Matx31d"): ("s_vec_add", vec)})
    ctx.funcs["triangulate_point"] = Fn("f_triangulate_point", [gm.c_ref(M31), gm.c_ref(M33), gm.c_ref(VEC3), gm.c_ref(VEC3)], VEC3)
    ctx.funcs["rec_new"] = Fn("s_rec_new", None, VOID)
    ctx.funcs["pow"] = Fn("s_pow", None, DOUBLE)
    ctx.funcs["saturate_cast_double"] = Fn("s_sat_double", None, DOUBLE)
    with gs.swapped(cxx_eval, "FuncTranslator", NpTranslator):
        params, _, body = gm.find_fn(rd("src", "misc.cpp"), r"cv::Vec3d triangulate_point\(")
        N_STMT[0] += body.count(";")
        srcs.append(translate_function(ctx, "f_triangulate_point", params, body, ret=VEC3, macros=macros))
        body = loop_text(rd("src", "cLocalMapping.cpp"))
        N_STMT[0] += body.count(";") - 1
        srcs.append(translate_function(ctx, "f_loop", LOOP_PARAMS, body, ret=VOID, macros=macros))
    return ctx, srcs, n_stmt + N_STMT[0]


def more_env(Matx):
    def m22_vec(A, x):
        return gf._vec([0.0 + A.a[i][0] * x.v[0] + A.a[i][1] * x.v[1] for i in range(2)])

    def get_minor(M, r0, c0):
        a = M.arr()
        return Matx(3, 3, [float(a[r0 + i, c0 + j]) for i in range(3) for j in range(3)])
    env = gs.more_env(Matx)
    env.update({"M22_": M22Obj, "M31_": lambda: gf._vec([0.0] * 3), "s_inv22": inv22, "s_m22_vec": m22_vec,
                "s_get_minor": get_minor, "s_sat_double": float})
    return env


def load(ref):
    """gen_fuse_ref.load with gen_sim3_ref's and this file's translations and stand-ins joined to its
    own.  The recording stand-ins (s_rec_new, s_pow, ...) are bound per run in run_pair."""
    saved = set(cxx_eval.VALUE_CLASSES)
    Matx = gm.make_refmath(ref)[1]
    box = {}
    late = {k: (lambda *a, k=k: box[k](*a)) for k in ("s_rec_new", "s_pow")}
    try:
        with gs.swapped(gf, "translate_all", translate_all), \
                gs.swapped(gf, "build_env", lambda ctx, rt_, extra: build_env(ctx, rt_, dict(extra, **more_env(Matx), **late))):
            G, R, Matx, _ = gf.load(ref)
    finally:
        cxx_eval.VALUE_CLASSES.clear()
        cxx_eval.VALUE_CLASSES.update(saved)
    return G, R, Matx, box


NAN = float("nan")


def run_pair(G, R, Matx, box, rig, kf1, kf2, matches12, nbytes, masked):
    """The translated loop on one (KF1, KF2) pair with vMatchedIndices in idx1 order
    (src/cORBmatcher.cpp:1140-1152) -> rows [n_matches, 13]: idx1, idx2, verdict, cos, z1, err1,
    z2, err2, dist1, dist2, x3D."""
    q = dict(pos=np.zeros((1, 3)), dist=np.ones((1, 2)), desc=np.zeros((1, nbytes), np.uint8),
             mask=np.zeros((1, nbytes), np.uint8) if masked else None)
    none = [np.full(len(k["kp_xy"]), -1, np.int32) for k in (kf1, kf2)]
    Wd = gf.World(G, R, Matx, rig, [kf1, kf2], q, np.zeros(1, np.int32), np.zeros(1, np.uint8), none,
                  [np.zeros(1, np.uint8)] * 2, q["desc"], nbytes, masked)
    sigma2 = np.asarray(rig["scale"], np.float64) ** 2
    cur = {}
    rows = []
    cams_d = [dict(c, p=c["a"], invp=c["pol"]) for c in rig["cams"]]
    for kf in Wd.kfs:
        kf.f["GetSigma2"] = lambda lv: float(sigma2[lv])
        for c, cam in enumerate(kf["camSystem"]["camModels"].v):
            def w2i(x, y, z, u, v, c=c):
                u[0], v[0] = R.world_to_img(cams_d[c], x, y, z)
                cur["z"].append(z)
            cam.f["WorldToImg"] = w2i
        w2c = kf["camSystem"].f["WorldToCamHom_fast"]
        kf["camSystem"].f["WorldToCamHom_fast"] = lambda c, p4, uv, w2c=w2c: (cur.__setitem__("x4", list(p4.v)), w2c(c, p4, uv))[1]
    env = G["f_loop"].__globals__
    dot0, norm0, sqrt0, tri0 = env["s_vec_dot"], env["s_cv__norm"], env["s_cv__sqrt"], G["f_triangulate_point"]

    def start():
        if cur:
            finish()
        cur.update(dot=None, norms=[], z=[], err=[], tri=False, in_tri=False, pow=False, new=None, x4=[NAN] * 3)

    def finish():
        z, err, nm = cur["z"], cur["err"], cur["norms"]
        if cur["new"] is not None:
            verdict = 1
        elif not cur["tri"]:
            verdict = 2
        elif len(z) == 1:
            verdict = 3 if not err else 4
        elif len(err) == 1:
            verdict = 5
        else:
            verdict = 7 if cur["pow"] else 6
        cos = cur["dot"] / (nm[0] * nm[1])
        rows.append([verdict, cos, z[0] if z else NAN, err[0] if err else NAN, z[1] if len(z) > 1 else NAN,
                     err[1] if len(err) > 1 else NAN, nm[2] if len(nm) > 2 else NAN, nm[3] if len(nm) > 3 else NAN]
                    + cur["x4"][:3])
        if cur["new"] is not None:
            assert cur["new"][0] == cur["x4"][:3]
        cur.clear()

    def dot(a, b):
        if not cur or not cur.get("in_tri"):
            start()                          # rayRot1.dot(rayRot2): once per iteration, before any `continue`
            cur["dot"] = dot0(a, b)
            return cur["dot"]
        return dot0(a, b)

    def norm(v):
        r = norm0(v)
        cur["norms"].append(r)
        return r

    def sqrt(x):
        r = sqrt0(x)
        cur["err"].append(r)
        return r

    def tri(*a):
        cur["tri"] = cur["in_tri"] = True
        r = tri0(*a)
        cur["in_tri"] = False
        return r

    def rec_new(x3d, idx1, idx2):
        cur["new"] = (list(x3d.v), int(idx1), int(idx2))

    def pw(x, y):
        cur["pow"] = True
        return math.pow(x, y)
    box["s_rec_new"], box["s_pow"] = rec_new, pw
    pairs = [(i, int(m)) for i, m in enumerate(matches12) if m >= 0]
    V = rt.Vector
    keys = lambda kf, idx: V(rt.KeyPoint, [kf["mvKeys"].v[k] for k in idx])  # noqa: E731
    rays = lambda kf, idx: V(lambda: gf._vec([0.0] * 3), [gf._vec(kf["rays"][k]) for k in idx])  # noqa: E731
    i1, i2 = [p[0] for p in pairs], [p[1] for p in pairs]
    Ow = [gf._vec(np.asarray(k["m_t"], np.float64).reshape(4, 4)[:3, 3]) for k in (kf1, kf2)]
    saved = {k: env[k] for k in ("s_vec_dot", "s_norm", "s_cv__norm", "s_sqrt", "s_cv__sqrt", "f_triangulate_point")}
    env.update(s_vec_dot=dot, s_norm=norm, s_cv__norm=norm, s_sqrt=sqrt, s_cv__sqrt=sqrt, f_triangulate_point=tri)
    try:
        G["f_loop"](Wd.kf_ptr[0], V(lambda: None, [Wd.kf_ptr[1]]), 0, Wd.kf_ptr[1], rays(kf1, i1), rays(kf2, i2),
                    keys(Wd.kfs[0], i1), keys(Wd.kfs[1], i2), V(rt.Pair, [rt.Pair(a, b) for a, b in pairs]),
                    Ow[0], Ow[1], float(np.linalg.norm(np.array(Ow[1].v) - np.array(Ow[0].v))), 1.0e-3,
                    math.cos(3.0 * 3.14159265358979323846 / 180.0), 6e-6, 25.0)
        if cur:
            finish()
    finally:
        env.update(saved)
    assert len(rows) == len(pairs), (len(rows), len(pairs))
    return np.array([[a, b] + r for (a, b), r in zip(pairs, rows)], np.float64).reshape(-1, 13)


KF_KEYS = ("kp_xy", "kp_octave", "kp_cam", "desc", "rays", "m_t", "pose6", "has_mp")


def near_threshold(rows):
    """Rows with an evaluated quantity within relative CRAFT_MARGIN of its threshold (absolute at 0)."""
    cos_th = math.cos(3.0 * 3.14159265358979323846 / 180.0)
    bad = np.zeros(len(rows), bool)
    with np.errstate(invalid="ignore"):
        for col, ths in ((3, (0.0, cos_th)), (4, (0.0,)), (5, (4.0,)), (6, (0.0,)), (7, (4.0,)), (8, (0.0, 25.0)), (9, (0.0, 25.0))):
            for th in ths:
                bad |= np.abs(rows[:, col] - th) <= CRAFT_MARGIN * (abs(th) if th else 1.0)
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(HERE, "newpoints_ref.npz"))
    a = ap.parse_args()
    from tests.test_newpoints_ref import SCENARIOS, make_scene
    G, R, Matx, box = load(a.ref)
    out = {"n_statements": np.int32(N_STMT[0]), "scenarios": np.array([s[0] for s in SCENARIOS])}
    seen = np.zeros(8, np.int64)
    for name, seed, n_per_cam, nbytes, masked, neighbours, kf2_first in SCENARIOS:
        rig, kf1, kf2s, truth = make_scene(seed, n_per_cam=n_per_cam, nbytes=nbytes, masked=masked, neighbours=neighbours)
        p = name + "_"
        out[p + "config"] = np.array([seed, n_per_cam, nbytes, int(masked), len(kf2s)], np.int32)
        out[p + "kf2_first"], out[p + "kind"] = np.array(kf2_first, np.uint8), kf1["kind"]
        for tag, kf in [("k1_", kf1)] + [("k2_%d_" % t, k) for t, k in enumerate(kf2s)]:
            for k in KF_KEYS + (("mask",) if masked else ()):
                out[p + tag + k] = kf[k]
        for t, kf2 in enumerate(kf2s):
            rows = run_pair(G, R, Matx, box, rig, kf1, kf2, truth[t], nbytes, masked)
            close = near_threshold(rows)
            if close.any():
                raise SystemExit("scenario %s, neighbour %d: rows %s lie within %g of a threshold: change the seed"
                                 % (name, t, rows[close, 0].astype(int).tolist(), CRAFT_MARGIN))
            out[p + "truth_%d" % t], out[p + "rows_%d" % t] = truth[t], rows
            cnt = np.bincount(rows[:, 2].astype(int), minlength=8)
            seen += cnt
            print(name, "neighbour", t, neighbours[t], "matches", len(rows), "verdicts 1..7", cnt[1:].tolist(), flush=True)
    if (seen[1:] == 0).any():
        raise SystemExit("verdicts %s never occur: change the seeds" % (np.flatnonzero(seen[1:] == 0) + 1).tolist())
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
