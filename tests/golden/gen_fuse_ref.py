"""Generate tests/golden/fuse_ref.npz: the three cORBmatcher::Fuse overloads, evaluated from the
reference TEXT on scripted keyframes of the Lafida rig (no reference source is stored: the fixture
holds numbers only).

Translated from /root/reference by tests/golden/cxx_eval.py (safe_exec, no builtins):
  cORBmatcher::Fuse(pKF, curKF, vpMapPoints, th)  (rule 0)   src/cORBmatcher.cpp:1265-1418
  cORBmatcher::Fuse(pKF, vpMapPoints, th)         (rule 1)   :1420-1567
  cORBmatcher::Fuse(pKF, Scw, vpPoints, th)       (rule 2)   :1570-1719
  cORBmatcher ctor (TH_LOW_), DescriptorDistance64[Masked]   :44-65, :2443-2477
  cMultiKeyFrame::GetFeaturesInArea                          src/cMultiKeyFrame.cpp:703-746
  cMultiKeyFrame::AddMapPoint, EraseMapPointMatch, ReplaceMapPointMatch, GetMapPoints,
      GetMapPoint                                            :273-304, :328-332
  cMapPoint::Replace, AddObservation, IsInKeyFrame, isBad, GetMinDistanceInvariance,
      GetMaxDistanceInvariance                    src/cMapPoint.cpp:208-250, :90-96, :447-451, :498-508
  cMultiCamSys_::WorldToCamHom_fast (Vec4d; the !flagMcMt branch runs)  src/cam_system_omni.cpp:92-112
  cCamModelGeneral_::isPointInMirrorMask                     src/cam_model_omni.cpp:165-180
and through tests/golden/gen_refmath.py (RefMath; refmath.npz pins them): cConverter::invMat,
cCamModelGeneral_::WorldToImg, CheckDistEpipolarLine, Skew, and with its translator
ComputeE(Trel) (include/misc.h:235-243).
Stand-ins, in this file:
  * cv::Vec / cv::Matx arithmetic as gen_mapside_ref.py states it (products and dot accumulate
    s = 0; s += a_k * b_k in order; cv::norm = sqrt of the in-order sum of squares; alpha * M and
    v /= a scale every element, the latter by 1. / a); Hom2R, Hom2T, Rt2Hom, toVec4d;
  * cMultiCamSys_::Get_MtMc, Get_MtMc_inv (include/cam_system_omni.h:162-176, the !flagMcMt
    branch: M_t * M_c[c] and invMat of it), Set_M_t, Get_M_t; the mirror masks of mcs_amd.synth;
  * the keyframe's grid (PosInGrid per keypoint in index order, which matcher_ref.npz pins for the
    frame constructor), keypoints, rays, descriptors, scale factors, GetCameraCenter
    (src/cMultiKeyFrame.cpp:159-165) as scripted data; std::set<cMapPoint*> as a Python set;
  * cMapPoint::ComputeDistinctiveDescriptors (src/cMapPoint.cpp:244) replaces the survivor's
    descriptor by a scripted row (`new_desc`), which is what makes a later target see the change;
    IncreaseFound / IncreaseVisible / cMap::EraseMapPoint do nothing.
The scenarios come from tests/test_fuse_ref.py (make_case), and every atan-dependent decision
keeps a margin of 1e-9 from its boundary, or the generator refuses the scenario: a projected pixel
from a rounding half, a floor / ceil argument of the cell range from an integer, |dx| - r and
|dy| - r from zero.  Recorded per scenario: every GetFeaturesInArea call (target, map point,
camera, u, v, r) and the list it returned, every GetMapPoint(bestIdx) of the tails, the ordered
AddObservation / Replace calls, nFused, and the map state after each target.

    python tests/golden/gen_fuse_ref.py [--ref /root/reference] [--out tests/golden/fuse_ref.npz]
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
import gen_matcher_ref as gm  # noqa: E402
from cxx_eval import BOOL, DOUBLE, INT, VOID, ClassSpec, Cls, Fn, PtrT, build_env, class_body, parse_members, translate_function  # noqa: E402
from safe_exec import safe_exec  # noqa: E402

INT_MAX = 2 ** 31 - 1
MARGIN = 1e-9
V, c_ref, m_ref, val, _sig = gm.V, gm.c_ref, gm.m_ref, gm.val, gm._sig
VEC2, VEC3, VEC4, MP, MKF = gm.VEC2, gm.VEC3, gm.VEC4, gm.MP, gm.MKF
M44, M33 = Cls("Matx44d"), Cls("Matx33d")
# (scenario, rule, seed, targets, queries, keypoints per camera, bytes, masked)
SCENARIOS = [("r0", 0, 201, 3, 140, 120, 32, False), ("r1", 1, 202, 3, 140, 120, 32, False),
             ("r2", 2, 203, 3, 140, 120, 32, False), ("r0m16", 0, 204, 1, 120, 120, 16, True),
             ("r0b64", 0, 205, 1, 120, 120, 64, False),
             # the same keyframes and crafted queries (craft_distances) under the float (rule 0) and the
             # double (rule 2) dist3D
             ("e0", 0, 206, 1, 120, 120, 32, False), ("e2", 2, 206, 1, 120, 120, 32, False)]
EDGE = ("e0", "e2")
# kinds of crafted queries: the distance exactly on the lower / upper bound, one ulp outside each,
# a lower bound between the float-rounded and the double distance, dist3D / minDistance exactly a
# scale factor, and a point mirrored through the rig centre (behind the cameras it was seen by)
CRAFT = ("lower_exact", "lower_ulp_out", "upper_exact", "upper_ulp_out", "float_flip", "ratio_is_scale", "behind",
         # craft_windows: a window clamped at each edge of the grid, one fully outside it, and one window
         # that holds keypoints at level - 2, level - 1, level and level + 1, the two admissible ones
         # at equal distance (the first in cell order wins) and the other two at distance 0
         "clamp_left", "clamp_right", "clamp_top", "clamp_bottom", "outside", "levels_and_tie")
EDGE_GRID = ((140, 10), (640, 470))    # mnMinX, mnMinY / mnMaxX, mnMaxY of the edge scenarios' keyframes
EDGE_PIXELS = {"clamp_left": (142.0, 240.0), "clamp_right": (638.0, 240.0), "clamp_top": (392.0, 12.0),
               "clamp_bottom": (392.0, 468.0), "outside": (131.0, 240.0), "levels_and_tie": (400.0, 250.0)}
N_MP = 400
SIM3_SCALE = 1.7


def translate_all(ref):
    ctx, mcpp, fcpp, macros, mf, om = gm.setup(ref)
    rd = lambda *p: open(os.path.join(ref, *p), encoding="latin-1").read()  # noqa: E731
    kcpp, kh, mph, mpcpp = rd("src", "cMultiKeyFrame.cpp"), rd("include", "cMultiKeyFrame.h"), \
        rd("include", "cMapPoint.h"), rd("src", "cMapPoint.cpp")
    r_int = val(INT)
    SET = Cls("set", (PtrT(MP),))
    for vc in ("mutex", "unique_lock"):
        cxx_eval.VALUE_CLASSES.add(vc)
    ctx.add_class(ClassSpec("mutex"))
    ctx.add_class(ClassSpec("unique_lock", ctor="Lock_", runtime_ctor=lambda *a: None))
    ctx.add_class(ClassSpec("cMap", {}, {"EraseMapPoint": _sig([val(PtrT(MP))], VOID)}))
    ctx.add_class(ClassSpec("set", {}, {"count": _sig([val(PtrT(MP))], INT), "insert": _sig([val(PtrT(MP))], VOID)},
                            ctor="Set_", runtime_ctor=lambda *a: None))
    at = Fn("s_matx_at", [r_int, r_int], DOUBLE)
    ctx.classes["Matx33d"].methods["()"] = at
    ctx.classes["Matx44d"].methods["()"] = at
    ctx.add_class(ClassSpec("Vec", {}, {"dot": Fn("s_vec_dot", [c_ref(VEC3)], DOUBLE)}))
    ctx.classes["cMultiCamSys_"].methods.update({
        "Set_M_t": _sig([val(M44)], VOID), "Get_M_t": _sig([], M44),
        "WorldToCamHom_fast": _sig([r_int, m_ref(VEC4), m_ref(VEC2)], BOOL)})
    MX = lambda r, c: Cls("Matx", (DOUBLE, r, c))  # noqa: E731
    ctx.add_class(ClassSpec("Matx", {}, {"()": at}, ctor="Matx_", runtime_ctor=lambda: None))
    cam, rig = ctx.classes["cCamModelGeneral_"], ctx.classes["cMultiCamSys_"]
    cam.fields["mirrorMasks"] = V(gm.MAT)
    cam.methods["WorldToImg"] = _sig([c_ref(DOUBLE)] * 3 + [m_ref(DOUBLE)] * 2, VOID)
    cam.methods["isPointInMirrorMask"] = _sig([c_ref(DOUBLE), c_ref(DOUBLE), r_int], BOOL)
    rig.fields.update({"flagMcMt": BOOL, "M_t": MX(4, 4), "M_c": V(MX(4, 4)), "MtMc": V(MX(4, 4)),
                       "MtMc_inv": V(MX(4, 4)), "camModels": V(Cls("cCamModelGeneral_"))})
    ctx.binops.update({("Matx", "*", "Matx"): ("s_matx_mul", lambda a, b: MX(a.args[1], b.args[2])),
                       ("Matx", "*", "Vec"): ("s_matx_mul", lambda a, b: MX(a.args[1], 1)),
                       ("Matx44d", "*", "Vec"): ("s_matx_mul", lambda a, b: MX(4, 1))})
    kf, mp = ctx.classes["cMultiKeyFrame"], ctx.classes["cMapPoint"]
    kf.fields.update(parse_members(ctx, class_body(kh, "cMultiKeyFrame")))
    mp.fields.update(parse_members(ctx, class_body(mph, "cMapPoint")))
    kf.methods.update({
        "GetScaleLevels": _sig([], INT), "GetScaleFactors": _sig([], V(DOUBLE)), "GetScaleFactor": _sig([r_int], DOUBLE),
        "GetCameraCenter": _sig([], VEC3), "GetKeyPointScaleLevel": _sig([c_ref(INT)], INT),
        "GetKeyPointRay": _sig([c_ref(INT)], VEC3), "HavingMasks": _sig([], BOOL),
        "GetFeaturesInArea": _sig([c_ref(INT), c_ref(DOUBLE), c_ref(DOUBLE), c_ref(DOUBLE)], V(INT)),
        "GetMapPoint": _sig([c_ref(INT)], PtrT(MP)), "AddMapPoint": _sig([val(PtrT(MP)), c_ref(INT)], VOID),
        "EraseMapPointMatch": _sig([c_ref(INT)], VOID), "ReplaceMapPointMatch": _sig([c_ref(INT), val(PtrT(MP))], VOID),
        "GetMapPoints": _sig([], SET)})
    mp.methods.update({
        "IsInKeyFrame": _sig([val(PtrT(MKF))], BOOL), "GetMaxDistanceInvariance": _sig([], DOUBLE),
        "GetMinDistanceInvariance": _sig([], DOUBLE), "GetNormal": _sig([], VEC3),
        "Replace": _sig([val(PtrT(MP))], VOID), "AddObservation": _sig([val(PtrT(MKF)), c_ref(INT)], VOID),
        "ComputeDistinctiveDescriptors": _sig([val(BOOL)], VOID), "GetDescriptor": _sig([], Cls("Mat")),
        "UpdateCurrentDescriptor": _sig([m_ref(Cls("Mat"))], VOID), "IncreaseFound": _sig([val(INT)], VOID),
        "IncreaseVisible": _sig([val(INT)], VOID)})
    same = lambda a, b: a  # noqa: E731
    ctx.binops.update({("Vec", "-", "Vec"): ("s_vec_sub", same), ("Matx44d", "*", "Matx44d"): ("s_matx_mul", same),
                       ("arith", "*", "Matx33d"): ("s_scale", lambda a, b: b),
                       ("arith", "*", "Vec"): ("s_scale", lambda a, b: b), ("iterator", "-", "iterator"): ("s_it_sub", INT)})
    for name, ret in [("norm", DOUBLE), ("cv::norm", DOUBLE), ("cConverter::Hom2R", M33), ("cConverter::Hom2T", VEC3),
                      ("cConverter::invMat", M44), ("cConverter::Rt2Hom", M44), ("cv::sqrt", DOUBLE), ("sqrt", DOUBLE)]:
        ctx.funcs[name] = Fn("s_" + re.sub(r"\W", "_", name), None, ret)
    ctx.funcs["lower_bound"] = ctx.funcs["std::lower_bound"] = Fn("s_lower_bound", None, lambda ts: ts[0])
    srcs, n_stmt = [], [0]

    def fn(pyname, text, pattern, this=None, ret=VOID, ctor=False):
        params, init, body = gm.find_fn(text, pattern)
        n_stmt[0] += body.count(";")
        srcs.append(translate_function(ctx, pyname, params, body, this_cls=this, ret=ret, macros=macros,
                                       init_text=init if ctor else None))
    fn("f_DescriptorDistance64", mcpp, r"int DescriptorDistance64\(", ret=INT)
    fn("f_DescriptorDistance64Masked", mcpp, r"int DescriptorDistance64Masked\(", ret=INT)
    fn("f_matcher_ctor", mcpp, r"cORBmatcher::cORBmatcher\(double nnratio", this=om, ctor=True)
    fn("f_fuse0", mcpp, r"int cORBmatcher::Fuse\(cMultiKeyFrame \*pKF,\s*cMultiKeyFrame \*curKF", this=om, ret=INT)
    fn("f_fuse1", mcpp, r"int cORBmatcher::Fuse\(cMultiKeyFrame\* pKF,\s*std::vector<cMapPoint\*> &vpMapPoints", this=om, ret=INT)
    fn("f_fuse2", mcpp, r"int cORBmatcher::Fuse\(cMultiKeyFrame \*pKF, cv::Matx44d Scw", this=om, ret=INT)
    fn("f_kf_GetFeaturesInArea", kcpp, r"std::vector<size_t> cMultiKeyFrame::GetFeaturesInArea\(", this=kf, ret=V(INT))
    fn("f_kf_AddMapPoint", kcpp, r"void cMultiKeyFrame::AddMapPoint\(", this=kf)
    fn("f_kf_EraseMapPointMatch", kcpp, r"void cMultiKeyFrame::EraseMapPointMatch\(const size_t", this=kf)
    fn("f_kf_ReplaceMapPointMatch", kcpp, r"void cMultiKeyFrame::ReplaceMapPointMatch\(", this=kf)
    fn("f_kf_GetMapPoints", kcpp, r"std::set<cMapPoint\*> cMultiKeyFrame::GetMapPoints\(", this=kf, ret=SET)
    fn("f_kf_GetMapPoint", kcpp, r"cMapPoint\* cMultiKeyFrame::GetMapPoint\(", this=kf, ret=PtrT(MP))
    fn("f_mp_Replace", mpcpp, r"void cMapPoint::Replace\(", this=mp)
    fn("f_mp_AddObservation", mpcpp, r"void cMapPoint::AddObservation\(", this=mp)
    fn("f_mp_IsInKeyFrame", mpcpp, r"bool cMapPoint::IsInKeyFrame\(", this=mp, ret=BOOL)
    fn("f_mp_isBad", mpcpp, r"bool cMapPoint::isBad\(", this=mp, ret=BOOL)
    fn("f_mp_GetMinDistanceInvariance", mpcpp, r"double cMapPoint::GetMinDistanceInvariance\(\)", this=mp, ret=DOUBLE)
    fn("f_mp_GetMaxDistanceInvariance", mpcpp, r"double cMapPoint::GetMaxDistanceInvariance\(\)", this=mp, ret=DOUBLE)
    fn("f_isPointInMirrorMask", rd("src", "cam_model_omni.cpp"), r"bool cCamModelGeneral_::isPointInMirrorMask\(", this=cam, ret=BOOL)
    fn("f_WorldToCamHom_fast", rd("src", "cam_system_omni.cpp"),
       r"bool cMultiCamSys_::WorldToCamHom_fast\(int c,\s*cv::Vec<double, 4>& pt4", this=rig, ret=BOOL)
    return ctx, srcs, n_stmt[0]


# ------------------------------------------------------------------------------ stand-ins
def _vec(xs):
    return rt.Vector(lambda: 0.0, [float(x) for x in xs])


class PySet:
    """std::set<cMapPoint*>: insert / count; copies are independent."""

    def __init__(self, items=()):
        self.s = set(items)

    def copy(self):
        return PySet(self.s)

    def __getitem__(self, k):
        return {"insert": self.s.add, "count": lambda p: 1 if p in self.s else 0}[k]


def load(ref):
    import gen_mapside_ref as gs
    ctx, srcs, n_stmt = translate_all(ref)
    R, Matx = gm.make_refmath(ref)

    def scale(a, X):
        if isinstance(X, rt.Vector):
            return _vec([x * a for x in X.v])
        r, c = X.arr().shape
        return Matx(r, c, [x * a for x in np.ravel(X.arr())])

    import gen_refmath
    compute_e, _, n_e = gen_refmath.translate(os.path.join(ref, "include", "misc.h"),
                                              "inline cv::Matx33d ComputeE(const cv::Matx44d& Trel", "ComputeE1",
                                              ["Trel"], env=R.env)          # include/misc.h:235-243, from the text
    n_stmt += n_e

    def matx_mul(a, b):
        if isinstance(b, rt.Vector):
            b = Matx(len(b.v), 1, b.v)
        return a * b

    def epi(ray1, ray2, E, th):
        return R.check_dist_epipolar_line(list(ray1.v), list(ray2.v), E.arr(), th)[0]

    def rt2hom(Rm, t):
        A = Rm.arr()
        return Matx(4, 4, [float(A[0, 0]), float(A[0, 1]), float(A[0, 2]), t.v[0], float(A[1, 0]), float(A[1, 1]),
                           float(A[1, 2]), t.v[1], float(A[2, 0]), float(A[2, 1]), float(A[2, 2]), t.v[2],
                           0.0, 0.0, 0.0, 1.0])
    extra = {
        "Lock_": lambda *a: None, "Set_": PySet, "s___builtin_popcountll": rt.popcount64, "c_INT_MAX": INT_MAX,
        "s_cvRound": rt.cv_round, "s_norm": gs.cv_norm, "s_cv__norm": gs.cv_norm, "s_vec_dot": gs.vec_dot,
        "s_vec_sub": lambda a, b: _vec([x - y for x, y in zip(a.v, b.v)]), "s_matx_mul": matx_mul, "Matx_": lambda: None,
        "s_matx_at": lambda m, i, j: m(i, j), "s_it_sub": lambda a, b: a - b, "s_lower_bound": gs.lower_bound,
        "s_scale": scale, "s_sqrt": math.sqrt, "s_cv__sqrt": math.sqrt, "s_ComputeE": compute_e,
        "s_CheckDistEpipolarLine": epi, "s_cConverter__invMat": R.env["invMat"], "s_cConverter__Rt2Hom": rt2hom,
        "s_cConverter__Hom2R": lambda M: Matx(3, 3, [float(M.arr()[i, j]) for i in range(3) for j in range(3)]),
        "s_cConverter__Hom2T": lambda M: _vec([M.arr()[i, 3] for i in range(3)]),
        "s_cConverter__toVec4d": lambda v: _vec(list(v.v) + [1.0]),
        "s_sort": rt.std_sort, "s_ComputeThreeMaxima": None, "s_HResClk__now": lambda: 0.0,
        "s_T_in_ms": lambda a, b: 0.0, "Matx33d_": lambda: Matx(3, 3), "Matx44d_": lambda: Matx(4, 4)}
    ctx.classes["Matx33d"].runtime_ctor = lambda: Matx(3, 3)
    ctx.classes["Matx44d"].runtime_ctor = lambda: Matx(4, 4)
    ctx.classes["set"].runtime_ctor = PySet
    env = build_env(ctx, rt, extra)
    G = safe_exec("\n".join(srcs), env, "<ref:cORBmatcher.cpp / cMultiKeyFrame.cpp / cMapPoint.cpp>")
    return G, R, Matx, n_stmt


class World:
    """The scripted map of one scenario: keyframes and map points whose state-changing methods are
    the translated reference functions, wrapped to record what the tails do."""

    def __init__(self, G, R, Matx, rig, targets, q, q_mp, mp_bad, kp_mp, in_kf, new_desc, nbytes, masked):
        self.G, self.rec_gfa, self.rec_get, self.rec_act, self.margin = G, [], [], [], np.inf
        self.cur_mp, self.cur_t, self.in_replace = -1, -1, False
        self.desc = {}                 # map point id -> its current descriptor row (queries only)
        C = len(rig["m_c"])
        cams_d = [dict(c, p=c["a"], invp=c["pol"]) for c in rig["cams"]]
        Mc = [Matx(4, 4, list(np.ravel(rig["m_c"][c]))) for c in range(C)]
        mirror = rig["mirror"]
        world = self

        def cam_obj(c):
            def w2i(x, y, z, u, v):
                u[0], v[0] = R.world_to_img(cams_d[c], x, y, z)
            cam = rt.Struct("cCamModelGeneral_", dict(mirrorMasks=rt.Vector(rt.Mat, [rt.Mat(mirror[c])]), WorldToImg=w2i))
            cam["isPointInMirrorMask"] = lambda u, v, pyr: G["f_isPointInMirrorMask"](cam, u, v, pyr)
            return cam
        cam_objs = [cam_obj(c) for c in range(C)]

        def make_rig(m_t):
            rig_ = rt.Struct("cMultiCamSys_", dict(
                flagMcMt=False, M_t=Matx(4, 4, list(np.ravel(m_t))), M_c=rt.Vector(lambda: None, list(Mc)),
                camModels=rt.Vector(lambda: None, cam_objs), GetNrCams=lambda: C, GetCamModelObj=lambda c: cam_objs[c]))

            def w2c(c, pt4, uv):               # the translated WorldToCamHom_fast (!flagMcMt branch)
                r = G["f_WorldToCamHom_fast"](rig_, c, pt4, uv)
                u, v = uv[0], uv[1]
                world.margin = min(world.margin, abs(abs(u - math.floor(u)) - 0.5), abs(abs(v - math.floor(v)) - 0.5))
                return r
            rig_.f.update(WorldToCamHom_fast=w2c, Get_MtMc=lambda c: rig_["M_t"] * Mc[c],
                          Get_MtMc_inv=lambda c: R.env["invMat"](rig_["M_t"] * Mc[c]),
                          Set_M_t=lambda M: rig_.f.__setitem__("M_t", M), Get_M_t=lambda: rig_["M_t"])
            return rig_
        from tests.test_fuse_ref import np_grid
        gp = rig["grid_params"]
        self.kfs, self.kf_ptr = [], []
        for t, tg in enumerate(targets):
            n = len(tg["kp_xy"])
            cells = np_grid(tg["kp_xy"], tg["kp_cam"], gp)
            grids = rt.Vector(lambda: None, [rt.Vector(lambda: None, [rt.Vector(lambda: None, [
                rt.Vector(lambda: 0, list(cells.get((c, ix, iy), []))) for iy in range(48)]) for ix in range(64)])
                for c in range(C)])
            keys = rt.Vector(rt.KeyPoint)
            for i in range(n):
                k = rt.KeyPoint()
                k["pt"] = rt.Point2f(float(tg["kp_xy"][i, 0]), float(tg["kp_xy"][i, 1]))
                k["octave"] = int(tg["kp_octave"][i])
                keys.v.append(k)
            k2c, k2l = rt.Map(lambda: 0), rt.Map(lambda: 0)
            first = {c: int(np.flatnonzero(tg["kp_cam"] == c)[0]) if (tg["kp_cam"] == c).any() else 0 for c in range(C)}
            for i in range(n):
                k2c.d[i] = int(tg["kp_cam"][i])
                k2l.d[i] = i - first[int(tg["kp_cam"][i])]

            def row(table, cam, i, tg=tg, first=first):
                r = first[cam] + int(i)
                assert tg["kp_cam"][r] == cam
                return rt.Ptr(np.ascontiguousarray(tg[table][r]).view("<u8").reshape(-1), 0)
            camsys = make_rig(tg["m_t"])
            f = dict(mMutexFeatures=None, mvpMapPoints=rt.Vector(lambda: None, [None] * n), mvKeys=keys, mGrids=grids,
                     mnMinX=rt.Vector(lambda: 0, [int(g[0]) for g in gp]), mnMinY=rt.Vector(lambda: 0, [int(g[1]) for g in gp]),
                     mfGridElementWidthInv=_vec(gp[:, 2]), mfGridElementHeightInv=_vec(gp[:, 3]),
                     mnGridCols=rt.Vector(lambda: 0, [64] * C), mnGridRows=rt.Vector(lambda: 0, [48] * C),
                     camSystem=camsys, keypoint_to_cam=k2c, cont_idx_to_local_cam_idx=k2l,
                     GetScaleLevels=lambda: len(rig["scale"]), GetScaleFactors=lambda: _vec(rig["scale"]),
                     GetScaleFactor=lambda lv: float(rig["scale"][lv]), HavingMasks=lambda: masked,
                     GetCameraCenter=lambda camsys=camsys: _vec([camsys["Get_M_t"]()(i, 3) for i in range(3)]),
                     GetKeyPointScaleLevel=lambda i, tg=tg: int(tg["kp_octave"][i]),
                     GetKeyPointRay=lambda i, tg=tg: _vec(tg["rays"][i]),
                     GetDescriptorRowPtr=lambda cam, i, row=row: row("desc", cam, i),
                     GetDescriptorMaskRowPtr=lambda cam, i, row=row: row("mask", cam, i))
            kf = rt.Struct("cMultiKeyFrame", f)
            for name in ("AddMapPoint", "EraseMapPointMatch", "ReplaceMapPointMatch", "GetMapPoints"):
                f[name] = (lambda name, kf: lambda *a: G["f_kf_" + name](kf, *a))(name, kf)

            def gfa(cam, x, y, r, kf=kf, t=t, tg=tg):
                out = G["f_kf_GetFeaturesInArea"](kf, cam, x, y, r)
                g = gp[cam]
                for a in ((x - g[0] - r) * g[2], (x - g[0] + r) * g[2], (y - g[1] - r) * g[3], (y - g[1] + r) * g[3]):
                    world.margin = min(world.margin, abs(a - round(a)))
                sel = np.flatnonzero(tg["kp_cam"] == cam)
                if len(sel):
                    kx = tg["kp_xy"][sel].astype(np.float64)
                    world.margin = min(world.margin, float(np.abs(np.abs(kx[:, 0] - x) - r).min()),
                                       float(np.abs(np.abs(kx[:, 1] - y) - r).min()))
                world.rec_gfa.append((t, world.cur_mp, cam, x, y, r, list(out.v)))
                return out

            def get_mp(idx, kf=kf, t=t):
                world.rec_get.append((t, world.cur_mp, int(idx)))
                return G["f_kf_GetMapPoint"](kf, idx)
            f["GetFeaturesInArea"], f["GetMapPoint"] = gfa, get_mp
            self.kfs.append(kf)
            self.kf_ptr.append(rt.Ptr(obj=kf))
        self.mps, self.mp_ptr = [], []
        rows = {int(m): i for i, m in reversed(list(enumerate(q_mp))) if m >= 0}
        for m in range(len(mp_bad)):
            i = rows.get(m)
            self.desc[m] = (q["desc"][i] if i is not None else new_desc[m]).copy()
            f = dict(mMutexFeatures=None, mMutexPos=None, mnId=m, mbBad=bool(mp_bad[m]), mnVisible=1, mnFound=1,
                     mpMap=gm.Obj(EraseMapPoint=lambda p: None),
                     mObservations=rt.Map(lambda: rt.Vector(lambda: 0), ordered=True),
                     mfMinDistance=float(q["dist"][i][0]) if i is not None else 1.0,
                     mfMaxDistance=float(q["dist"][i][1]) if i is not None else 2.0,
                     GetWorldPos=(lambda m=m, i=i: (setattr(world, "cur_mp", m), _vec(q["pos"][i]))[1]),
                     GetNormal=lambda: _vec([0.0, 0.0, 1.0]),
                     GetDescriptorPtr=lambda m=m: rt.Ptr(np.ascontiguousarray(world.desc[m]).view("<u8").reshape(-1), 0),
                     GetDescriptorMaskPtr=(lambda i=i: rt.Ptr(np.ascontiguousarray(q["mask"][i]).view("<u8").reshape(-1), 0))
                     if masked and i is not None else (lambda: None),
                     ComputeDistinctiveDescriptors=lambda hm, m=m: world.desc.__setitem__(m, new_desc[m].copy()),
                     GetDescriptor=lambda: None, UpdateCurrentDescriptor=lambda d: None,
                     IncreaseFound=lambda n: None, IncreaseVisible=lambda n: None)
            mp = rt.Struct("cMapPoint", f)
            for name in ("IsInKeyFrame", "isBad", "GetMinDistanceInvariance", "GetMaxDistanceInvariance"):
                f[name] = (lambda name, mp: lambda *a: G["f_mp_" + name](mp, *a))(name, mp)

            def add_obs(pKF, idx, mp=mp, m=m):
                if not world.in_replace:     # Replace's own AddObservation calls are its effect, not a tail action
                    world.rec_act.append((world.cur_t, 0, m, int(idx), m))
                return G["f_mp_AddObservation"](mp, pKF, idx)

            def replace(other, mp=mp, m=m):
                world.rec_act.append((world.cur_t, 1, m, world.rec_get[-1][2], int(rt.deref(other)["mnId"])))
                world.in_replace = True
                G["f_mp_Replace"](mp, other)
                world.in_replace = False
            f["AddObservation"], f["Replace"] = add_obs, replace
            self.mps.append(mp)
            self.mp_ptr.append(rt.Ptr(obj=mp))
        for t in range(len(targets)):        # the scripted slots and observations
            for k, m in enumerate(kp_mp[t]):
                if m >= 0:
                    self.kfs[t]["mvpMapPoints"].v[k] = self.mp_ptr[m]
                    if in_kf[t][m]:
                        G["f_mp_AddObservation"](self.mps[m], self.kf_ptr[t], k)

    def state(self, t):
        slots = np.array([-1 if p is None else rt.deref(p)["mnId"] for p in self.kfs[t]["mvpMapPoints"].v], np.int32)
        bad = np.array([mp["mbBad"] for mp in self.mps], np.uint8)
        inkf = np.array([mp["mObservations"].m_count(self.kf_ptr[t]) for mp in self.mps], np.uint8)
        return slots, bad, inkf


def _search(f, x0, want, span=4096):
    """A double near x0 with f(x) == want (f monotone), or None."""
    lo = hi = x0
    for _ in range(span):
        if f(lo) == want:
            return lo
        if f(hi) == want:
            return hi
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
    return None


def craft_distances(q, m_t, scale):
    """Rewrites the distance ranges (and one position) of the first queries so that they sit on the
    boundaries listed in CRAFT; none of them passes through atan.  -> [(query, kind index)]."""
    Ow = [float(m_t[i, 3]) for i in range(3)]
    done = []
    for i, kind in enumerate(CRAFT[:7]):
        if kind == "behind":
            q["pos"][i] = 2.0 * np.array(Ow) - q["pos"][i]
            done.append((i, CRAFT.index(kind)))
            continue
        PO = [float(q["pos"][i][k]) - Ow[k] for k in range(3)]
        d = math.sqrt(PO[0] * PO[0] + PO[1] * PO[1] + PO[2] * PO[2])
        df = float(np.float32(d))
        lo, hi = d / 1.7, d * 3.0
        if kind == "lower_exact":
            lo = _search(lambda x: 0.8 * x, d / 0.8, d)
        elif kind == "lower_ulp_out":
            x = _search(lambda x: 0.8 * x, d / 0.8, d)
            lo = None if x is None else _search(lambda x: 0.8 * x, x, float(np.nextafter(d, np.inf)))
        elif kind == "upper_exact":
            lo, hi = d / 3.0, _search(lambda x: 1.2 * x, d / 1.2, d)
        elif kind == "upper_ulp_out":
            x = _search(lambda x: 1.2 * x, d / 1.2, d)
            lo, hi = d / 3.0, None if x is None else _search(lambda x: 1.2 * x, x, float(np.nextafter(d, -np.inf)))
        elif kind == "float_flip":
            a, b = min(d, df), max(d, df)
            lo = (a + (b - a) / 2) / 0.8
            if not (a < 0.8 * lo <= b) or a == b:
                lo = None
        elif kind == "ratio_is_scale":
            lo = _search(lambda x: -(d / (0.8 * x)), d / (0.8 * float(scale[3])), -float(scale[3]))
        if lo is None or hi is None:
            continue
        q["dist"][i] = (lo, hi)
        done.append((i, CRAFT.index(kind)))
    return done


def craft_windows(rig, tg, q, first):
    """Rewrites queries first.. so that, in camera 0 of target tg, they project onto EDGE_PIXELS
    (along the pixel's bearing ray, depth 2) with a range that predicts level 1 (level 3 for
    levels_and_tie), and moves the target's keypoints 0..3 into one cell around the last pixel
    with octaves 1, 2, 3, 4.  -> [(query, kind index)]."""
    from mcs_amd import synth
    from tests.test_fuse_ref import _flip
    M = tg["m_t"] @ rig["m_c"][0]
    done = []
    for n, kind in enumerate(CRAFT[7:]):
        i = first + n
        u, v = EDGE_PIXELS[kind]
        assert rig["mirror"][0][int(v), int(u)] > 0 and tg["kp_cam"][3] == 0
        ray = np.array(synth.img_to_world(rig["cams"][0], np.float64(u), np.float64(v)), np.float64)
        q["pos"][i] = M[:3, :3] @ (ray * 2.0) + M[:3, 3]
        d = float(np.linalg.norm(q["pos"][i] - tg["m_t"][:3, 3]))
        ratio = 0.95 * float(rig["scale"][3]) if kind == "levels_and_tie" else 1.1
        q["dist"][i] = (d / (0.8 * ratio), d * 3.0)
        if kind == "levels_and_tie":
            rng = np.random.default_rng(7)
            near = _flip(q["desc"][i], 5, rng)
            for k, (dx, dy, octave) in enumerate(((-0.5, -0.5, 1), (0.5, -0.5, 2), (-0.5, 0.5, 3), (0.5, 0.5, 4))):
                tg["kp_xy"][k] = (u + dx, v + dy)
                tg["kp_octave"][k] = octave
                tg["desc"][k] = near if octave in (2, 3) else q["desc"][i]
                tg["rays"][k] = synth.img_to_world(rig["cams"][0], np.float64(u + dx), np.float64(v + dy))
        done.append((i, 7 + n))
    return done


def scenario_inputs(name, rule, seed, T, nq, n_per_cam, nbytes, masked):
    """The scripted keyframes, map points and map state of one scenario (also stored in the fixture)."""
    from tests.test_fuse_ref import make_case, np_sim3_to_mt
    rig, targets, q = make_case(seed=seed, T=T, nq=nq, n_per_cam=n_per_cam, nbytes=nbytes, masked=masked)
    if name in EDGE:
        from mcs_amd import window
        rig["grid_params"] = window.grid_params([EDGE_GRID[0]] * 3, [EDGE_GRID[1]] * 3)
    rng = np.random.default_rng(seed + 1000)
    q_mp = rng.permutation(N_MP)[:nq].astype(np.int32)
    if rule != 2:                                       # rule 2 dereferences every point (:1601)
        q_mp[rng.choice(nq, 6, replace=False)] = -1
    q_mp[5] = q_mp[4]                                   # the same map point at two keypoints
    q["pos"][5], q["dist"][5], q["desc"][5] = q["pos"][4], q["dist"][4], q["desc"][4]
    if masked:
        q["mask"][5] = q["mask"][4]
    mp_bad = (rng.random(N_MP) < 0.05).astype(np.uint8)
    kp_mp, in_kf, scw = [], [], []
    for tg in targets:
        n_kp = len(tg["kp_xy"])
        slots = np.full(n_kp, -1, np.int32)
        own = rng.choice(n_kp, n_kp // 2, replace=False)
        slots[own] = rng.permutation(N_MP)[:len(own)]
        obs = np.zeros(N_MP, np.uint8)
        obs[slots[slots >= 0]] = 1
        obs[mp_bad != 0] = 0                            # an occupied slot whose point is bad observes nothing
        kp_mp.append(slots)
        in_kf.append(obs)
        S = np.linalg.inv(tg["m_t"])
        S[:3] *= SIM3_SCALE
        scw.append(S)
        if rule == 2 or name in EDGE:
            tg["m_t"] = np_sim3_to_mt(S)
    if name in EDGE:
        q["crafted"] = craft_distances(q, targets[0]["m_t"], rig["scale"]) + craft_windows(rig, targets[0], q, 7)
        q_mp[:len(CRAFT)] = np.setdiff1d(np.arange(N_MP), np.concatenate([q_mp, kp_mp[0]]))[:len(CRAFT)]   # fresh, good points
        mp_bad[q_mp[:len(CRAFT)]] = 0
    new_desc = rng.integers(0, 256, (N_MP, nbytes), dtype=np.uint8)
    return rig, targets, q, q_mp, mp_bad, kp_mp, in_kf, new_desc, scw


def run_scenario(G, R, Matx, sc, out):
    name, rule, seed, T, nq, n_per_cam, nbytes, masked = sc
    rig, targets, q, q_mp, mp_bad, kp_mp, in_kf, new_desc, scw = scenario_inputs(*sc)
    W = World(G, R, Matx, rig, targets, q, q_mp, mp_bad, kp_mp, in_kf, new_desc, nbytes, masked)
    Mo = G["Matcher_"]()
    G["f_matcher_ctor"](Mo, 0.8, False, nbytes, masked)
    th = {0: 2.5, 1: 3.0, 2: 4.0}[rule]
    pts = rt.Vector(lambda: None, [W.mp_ptr[m] if m >= 0 else None for m in q_mp])
    cur = rt.Ptr(obj=rt.Struct("cMultiKeyFrame", dict(
        GetKeyPointRay=lambda i: _vec(q["rays"][i]),
        camSystem=gm.Obj(Get_MtMc_inv=lambda c: R.env["invMat"](Matx(4, 4, list(np.ravel(q["m_t"]))) *
                                                               Matx(4, 4, list(np.ravel(rig["m_c"][c]))))))))
    p = name + "_"
    n_fused = []
    for t in range(T):
        W.cur_t = t
        if rule == 0:
            n_fused.append(G["f_fuse0"](Mo, W.kf_ptr[t], cur, pts, th))
        elif rule == 1:
            n_fused.append(G["f_fuse1"](Mo, W.kf_ptr[t], pts, th))
        else:
            n_fused.append(G["f_fuse2"](Mo, W.kf_ptr[t], Matx(4, 4, list(np.ravel(scw[t]))), pts, th))
            got = W.kfs[t]["camSystem"]["Get_M_t"]().arr()
            assert np.array_equal(got, targets[t]["m_t"]), "rule 2: M_t from Scw differs from the restatement"
        slots, bad, inkf = W.state(t)
        out[p + "end%d_slots" % t], out[p + "end%d_bad" % t], out[p + "end%d_in_kf" % t] = slots, bad, inkf
    if not W.margin > MARGIN:
        raise SystemExit("scenario %s: a decision lies within %g of its boundary (margin %g): change the seed"
                         % (name, MARGIN, W.margin))
    out[p + "config"] = np.array([rule, T, nq, nbytes, int(masked), int(Mo["TH_LOW_"])], np.int32)
    out[p + "th"], out[p + "margin"] = np.float64(th), np.float64(W.margin)
    out[p + "n_fused"] = np.array(n_fused, np.int32)
    out[p + "actions"] = np.array(W.rec_act, np.int32).reshape(-1, 5)
    out[p + "get"] = np.array(W.rec_get, np.int32).reshape(-1, 3)
    out[p + "gfa_key"] = np.array([g[:3] for g in W.rec_gfa], np.int32).reshape(-1, 3)
    out[p + "gfa_xyr"] = np.array([g[3:6] for g in W.rec_gfa], np.float64).reshape(-1, 3)
    out[p + "gfa_ptr"] = np.concatenate([[0], np.cumsum([len(g[6]) for g in W.rec_gfa])]).astype(np.int32)
    out[p + "gfa_list"] = np.array([k for g in W.rec_gfa for k in g[6]], np.int32)
    for k in ("pos", "dist", "desc", "rays", "m_t") + (("mask",) if masked else ()):
        out[p + "q_" + k] = q[k]
    out[p + "q_mp"], out[p + "mp_bad"], out[p + "new_desc"] = q_mp, mp_bad, new_desc
    if name in EDGE:
        out[p + "crafted"] = np.array(q["crafted"], np.int32).reshape(-1, 2)
        out[p + "grid_params"] = rig["grid_params"]
    for t, tg in enumerate(targets):
        for k in ("kp_xy", "kp_octave", "kp_cam", "desc", "rays", "m_t") + (("mask",) if masked else ()):
            out[p + "t%d_%s" % (t, k)] = tg[k]
        out[p + "t%d_kp_mp" % t], out[p + "t%d_in_kf" % t], out[p + "t%d_scw" % t] = kp_mp[t], in_kf[t], scw[t]
    return W


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(HERE, "fuse_ref.npz"))
    a = ap.parse_args()
    G, R, Matx, n_stmt = load(a.ref)
    out = {"n_statements": np.int32(n_stmt), "scenarios": np.array([s[0] for s in SCENARIOS])}
    for sc in SCENARIOS:
        W = run_scenario(G, R, Matx, sc, out)
        print(sc[0], "nFused", out[sc[0] + "_n_fused"].tolist(), "actions", len(W.rec_act), "windows", len(W.rec_gfa),
              "margin %.3g" % W.margin, flush=True)
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
