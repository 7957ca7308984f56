"""Generate tests/golden/bow_ref.npz: the reference's two SearchByBoW overloads, evaluated from
their TEXT (no reference source is stored: the fixture holds numbers only).

Translated from the reference checkout by tests/golden/cxx_eval.py (setup shared with
gen_matcher_ref.py; safe_exec runs the result with no builtins):
  SearchByBoW(cMultiKeyFrame*, cMultiFrame&, ...)       src/cORBmatcher.cpp:179-323   (overload A)
  SearchByBoW(cMultiKeyFrame*, cMultiKeyFrame*, ...)    src/cORBmatcher.cpp:885-966   (overload B)
  ComputeThreeMaxima                                    src/cORBmatcher.cpp:2399-2441
  cORBmatcher ctor (TH_LOW_), DescriptorDistance64[Masked]   :44-65, :2443-2477
Stand-ins, registered here (cxx_eval / cxx_rt / safe_exec are imported unchanged):
  * DBoW2::FeatureVector is `class FeatureVector : public std::map<NodeId, std::vector<unsigned
    int> >` (ThirdParty/DBoW2/DBoW2/FeatureVector.h): the two names are expanded to that map type
    by the translator's macro table;
  * std::map::lower_bound (used at :294 / :298) is not in the translator's map runtime: FeatVec
    below supplies it with std::map semantics (first element whose key is not less than k, else
    end()), and the translator's method table is extended by that one entry;
  * cMapPoint / cMultiKeyFrame / cMultiFrame are scripted: map points (some absent, some bad),
    keypoints with angles, descriptors per camera, index maps, FeatureVectors.
Every distance the reference computes, every cvRound it takes and the ComputeThreeMaxima call
are recorded; main() asserts from those records that each scenario contains the cases the tests
are about (see `require`), so the fixture cannot go trivial.

    python tests/golden/gen_bow_ref.py [--ref /root/reference] [--out bow_ref.npz]
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cxx_eval  # noqa: E402
import cxx_rt as rt  # noqa: E402
import gen_matcher_ref as gm  # noqa: E402
from cxx_eval import (BOOL, INT, VOID, Cls, E, Fn, PtrT, Unsupported, build_env,  # noqa: E402
                      translate_function)
from safe_exec import safe_exec  # noqa: E402

NC = 3
INT_MAX = 2 ** 31 - 1
V = gm.V
FV_T = Cls("map", (INT, V(INT)))          # DBoW2::FeatureVector


# ------------------------------------------------------------------------------ lower_bound
class FeatVec(rt.Map):
    """std::map<NodeId, std::vector<unsigned>> with lower_bound (std::map semantics)."""
    __slots__ = ()

    def __init__(self, fac=None):
        rt.Map.__init__(self, fac or (lambda: rt.Vector(lambda: 0)), ordered=True)

    def copy(self):
        m = FeatVec(self.fac)
        m.d = {k: rt.cp(v) for k, v in self.d.items()}
        return m

    def __getitem__(self, k):
        if isinstance(k, str) and k == "lower_bound":
            return self.m_lower_bound
        return rt.Map.__getitem__(self, k)

    def m_lower_bound(self, k):
        for key in self.keys():
            if not key < k:
                return rt.MapIt(self, key)
        return self.m_end()


_base_method_call = cxx_eval.FuncTranslator.method_call


def _method_call(self, code, oty, mname, targs, args):
    if isinstance(oty, Cls) and oty.name == "map" and mname == "lower_bound":
        es = [self.ex(a) for a in args]
        return E("%s['lower_bound'](%s)" % (code, self.conv(es[0], oty.args[0])), Cls("iterator", (oty,)))
    return _base_method_call(self, code, oty, mname, targs, args)


def make_fv(node, ptr, feat):
    fv = FeatVec()
    for j, nd in enumerate(node):
        fv.d[int(nd)] = rt.Vector(lambda: 0, [int(x) for x in feat[ptr[j]:ptr[j + 1]]])
    return fv


# ------------------------------------------------------------------------------ translation
def load(ref):
    ctx, mcpp, fcpp, macros, mf, om = gm.setup(ref)
    cxx_eval.FuncTranslator.method_call = _method_call
    macros = dict(macros)
    macros["DBoW2"] = (None, cxx_eval.tokenize("std"))
    macros["FeatureVector"] = (None, cxx_eval.tokenize("map<unsigned int, vector<unsigned int> >"))
    mf.fields["mFeatVec"] = FV_T
    kf = ctx.classes["cMultiKeyFrame"]
    kf.methods["GetFeatureVector"] = gm._sig([], FV_T)
    kf.methods["GetKeyPoint"] = gm._sig([gm.c_ref(INT)], gm.KP)
    kf.methods["GetAllDescriptors"] = gm._sig([], V(gm.MAT))
    kf.methods["GetAllDescriptorMasks"] = gm._sig([], V(gm.MAT))
    ctx.funcs["ComputeThreeMaxima"] = Fn("f_ComputeThreeMaxima", [gm.val(Cls("carray", (V(INT),))), gm.c_ref(INT),
                                                                  gm.m_ref(INT), gm.m_ref(INT), gm.m_ref(INT)], VOID)
    srcs, n_stmt = [], [0]

    def fn(pyname, pattern, this=None, ret=VOID, ctor=False):
        params, init, body = gm.find_fn(mcpp, pattern)
        n_stmt[0] += body.count(";")
        srcs.append(translate_function(ctx, pyname, params, body, this_cls=this, ret=ret, macros=macros,
                                       init_text=init if ctor else None))
    fn("f_DescriptorDistance64", r"int DescriptorDistance64\(", ret=INT)
    fn("f_DescriptorDistance64Masked", r"int DescriptorDistance64Masked\(", ret=INT)
    fn("f_matcher_ctor", r"cORBmatcher::cORBmatcher\(double nnratio", this=om, ctor=True)
    fn("f_ComputeThreeMaxima", r"void cORBmatcher::ComputeThreeMaxima\(")
    fn("f_bow_a", r"int cORBmatcher::SearchByBoW\(cMultiKeyFrame\* pKF,\s*cMultiFrame &F", this=om, ret=INT)
    fn("f_bow_b", r"int cORBmatcher::SearchByBoW\(cMultiKeyFrame \*pKF1,\s*cMultiKeyFrame \*pKF2", this=om, ret=INT)
    import re
    histo = int(re.search(r"const int cORBmatcher::HISTO_LENGTH\s*=\s*(\d+)\s*;", mcpp).group(1))
    log = Log()
    extra = {"s_cvRound": log.cv_round, "s___builtin_popcountll": rt.popcount64, "c_INT_MAX": INT_MAX,
             "s_sort": rt.std_sort, "s_HResClk__now": lambda: 0.0, "s_T_in_ms": lambda a, b: 0.0}
    env = build_env(ctx, rt, extra)
    G = safe_exec("\n".join(srcs), env, "<ref:cORBmatcher.cpp SearchByBoW>")
    for name in ("f_DescriptorDistance64", "f_DescriptorDistance64Masked"):
        G[name] = log.wrap_dist(G[name])
    G["f_ComputeThreeMaxima"] = log.wrap_maxima(G["f_ComputeThreeMaxima"])
    return G, log, n_stmt[0], histo, srcs


class Log:
    """What the reference computed during one call: per query the (candidate, distance) list in
    its own order, every cvRound, the ComputeThreeMaxima call."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.queries, self.rounds, self.maxima = [], [], None
        self.pending = None

    def query(self, idx):
        self.queries.append((idx, []))

    def cand(self, idx):
        self.pending = idx

    def wrap_dist(self, f):
        def g(*a):
            d = f(*a)
            self.queries[-1][1].append((self.pending, d))
            return d
        return g

    def cv_round(self, x):
        r = rt.cv_round(x)
        self.rounds.append((float(x), r))
        return r

    def wrap_maxima(self, f):
        def g(histo, L, i1, i2, i3):
            sizes = [histo[i].m_size() for i in range(L)]
            f(histo, L, i1, i2, i3)
            self.maxima = (sizes, [c[0] for c in (i1, i2, i3)])
        return g


class LogMat(rt.Mat):
    """A per-camera descriptor Mat of F whose row reads name the candidate."""
    __slots__ = ("log", "base")

    def m_ptr_uint64_t(self, row):
        if self.log is not None:
            self.log.cand(self.base + row)
        return rt.Mat.m_ptr_uint64_t(self, row)


def split_cams(n):
    per = [n // NC + (1 if c < n % NC else 0) for c in range(NC)]
    return np.concatenate([[0], np.cumsum(per)]).astype(int)


def index_maps(n):
    off = split_cams(n)
    k2c, loc = rt.Map(lambda: 0), rt.Map(lambda: 0)
    for c in range(NC):
        for i in range(off[c], off[c + 1]):
            k2c.d[i] = c
            loc.d[i] = i - off[c]
    return off, k2c, loc


def kf_standin(log, role, desc, dmask, present, bad, angle=None, fv=None):
    """cMultiKeyFrame: role 'query' (its row reads open a query record) or 'cand'."""
    n, nbytes = desc.shape
    off, k2c, loc = index_maps(n)
    words = gm.desc_words(desc)
    mwords = gm.desc_words(dmask) if dmask is not None else None
    wpr = nbytes // 8
    mps = []
    for i in range(n):
        mps.append(rt.Ptr(obj=gm.Obj(id=i, isBad=(lambda b=bool(bad[i]): b))) if present[i] else None)

    def row(c, i):
        g = int(off[c]) + i
        (log.query if role == "query" else log.cand)(g)
        return rt.Ptr(words, g * wpr)

    def kp(i):
        k = rt.KeyPoint()
        k["angle"] = float(angle[i]) if angle is not None else -1.0
        return k
    mats = lambda a: rt.Vector(rt.Mat, [rt.Mat(np.array(a[off[c]:off[c + 1]], np.uint8)) for c in range(NC)])  # noqa: E731
    return gm.Obj(keypoint_to_cam=k2c, cont_idx_to_local_cam_idx=loc,
                  GetMapPointMatches=lambda: rt.Vector(lambda: None, list(mps)),
                  GetFeatureVector=lambda: fv.copy(), GetKeyPoint=kp,
                  GetDescriptorRowPtr=row,
                  GetDescriptorMaskRowPtr=lambda c, i: rt.Ptr(mwords, (int(off[c]) + i) * wpr),
                  GetAllDescriptors=lambda: mats(desc),
                  GetAllDescriptorMasks=lambda: mats(dmask if dmask is not None else np.zeros_like(desc)))


def frame_standin(G, log, desc, dmask, angle, fv):
    """cMultiFrame with the members SearchByBoW reads (:185, :198, :239-245, :274)."""
    n = len(desc)
    off, k2c, loc = index_maps(n)
    M = G["MultiFrame_"]()
    M["keypoint_to_cam"], M["cont_idx_to_local_cam_idx"] = k2c, loc
    M["mvpMapPoints"] = rt.Vector(lambda: None, [None] * n)
    M["mFeatVec"] = fv

    def mats(a):
        out = []
        for c in range(NC):
            m = rt.Mat(np.array(a[off[c]:off[c + 1]], np.uint8).reshape(-1, desc.shape[1]))
            lm = LogMat(m.buf, m.r0, m.c0, m.rows, m.cols)
            lm.log, lm.base = log, int(off[c])
            out.append(lm)
        return rt.Vector(rt.Mat, out)
    M["mDescriptors"] = mats(desc)
    M["mDescriptorMasks"] = mats(dmask if dmask is not None else np.zeros_like(desc))
    kps = []
    for i in range(n):
        k = rt.KeyPoint()
        k["angle"] = float(angle[i])
        kps.append(k)
    M["mvKeys"] = rt.Vector(rt.KeyPoint, kps)
    return M


# ------------------------------------------------------------------------------ scenario data
def flip_bits(d, nbits, rng, allowed=None):
    bits = np.unpackbits(d.copy())
    pool = np.arange(bits.size) if allowed is None else np.flatnonzero(allowed)
    if nbits:
        bits[rng.choice(pool, nbits, replace=False)] ^= 1
    return np.packbits(bits)


def rand_masks(rng, n, nbytes):
    return np.packbits((rng.random((n, nbytes * 8)) < 0.85).astype(np.uint8), axis=1)


def both_set(m1, m2):
    return np.unpackbits(m1 & m2).astype(bool)


def csr(nodes_of, order=None):
    """FeatureVector of a per-keypoint node array (-1 = in no node): ascending nodes, features
    in feature order (what TemplatedVocabulary::transform builds, TemplatedVocabulary.h:1170-1190)."""
    ids = sorted(set(int(x) for x in nodes_of if x >= 0))
    ptr, feat = [0], []
    for nd in ids:
        feat += [i for i in range(len(nodes_of)) if nodes_of[i] == nd]
        ptr.append(len(feat))
    return np.array(ids, np.uint32), np.array(ptr, np.int32), np.array(feat, np.uint32)


def scenario_a(seed, nbytes, masked, th_low, orient, n=360):
    """360 vs 360 keypoints in 4 shared nodes (130 / 100 / 70 / 40 keyframe keypoints) plus node
    40 only in the keyframe (the highest id) and node 2 only in the frame (the lowest)."""
    rng = np.random.default_rng(seed)
    kd = rng.integers(0, 256, (n, nbytes), dtype=np.uint8)
    km = rand_masks(rng, n, nbytes) if masked else None
    fm = rand_masks(rng, n, nbytes) if masked else None
    sizes = [(11, 130), (17, 100), (23, 70), (31, 40), (40, 20)]
    perm = rng.permutation(n)
    knode = np.zeros(n, np.int64)
    o = 0
    for nd, s in sizes:
        knode[perm[o:o + s]] = nd
        o += s
    present = rng.random(n) < 0.88
    bad = rng.random(n) < 0.05
    L = [i for i in range(n) if knode[i] == 11]          # node 11 in list order
    special = {k: L[p] for k, p in (("dup", 3), ("ratio", 5), ("u", 8), ("v", 9), ("th", 12))}
    for i in special.values():
        present[i], bad[i] = True, False
    kd[special["v"]] = flip_bits(kd[special["u"]], 2, rng)
    # F: keypoint i < 300 is keyframe keypoint part[i] seen again, the rest is new
    part = rng.permutation(n)[:300]
    # the specials keep a partner
    missing = [i for i in special.values() if i not in set(part.tolist())]
    for j, i in enumerate(missing):
        cand = [p for p in range(300) if part[p] not in special.values()]
        part[cand[j]] = i
    fnode = np.full(n, -1, np.int64)
    fd = rng.integers(0, 256, (n, nbytes), dtype=np.uint8)
    for i in range(300):
        k = int(part[i])
        fd[i] = flip_bits(kd[k], int(rng.integers(0, 41)), rng)
        fnode[i] = 2 if knode[k] == 40 else knode[k]
    extras = list(range(300, n))
    fnode[extras[:6]] = 11
    fnode[extras[6:]] = rng.choice([11, 17, 23, 31], len(extras) - 6)
    pf = {int(part[i]): i for i in range(300)}
    ok = lambda a, b: both_set(km[a], fm[b]) if masked else None  # noqa: E731
    x = special["dup"]                                   # two exact copies: best == best2 == 0
    fd[pf[x]] = kd[x]
    fd[extras[0]] = kd[x]
    if masked:
        fm[extras[0]] = fm[pf[x]]
    y = special["ratio"]                                 # 10 vs 12 bits: the ratio test fails
    fd[pf[y]] = flip_bits(kd[y], 10, rng, ok(y, pf[y]))
    fd[extras[1]] = flip_bits(kd[y], 12, rng, ok(y, extras[1]))
    u, v = special["u"], special["v"]                    # v's nearest is taken by u
    fd[pf[u]] = flip_bits(kd[u], 1, rng, ok(u, pf[u]))
    fd[pf[v]] = flip_bits(kd[v], 20, rng, ok(v, pf[v]))
    t = special["th"]                                    # exactly TH_LOW_
    fd[pf[t]] = flip_bits(kd[t], th_low, rng, ok(t, pf[t]))
    ka = np.zeros(n, np.float32)
    fa = rng.integers(0, 300, n).astype(np.float32)
    if orient:
        # rot per pair: 3 (bin 0), 15 (the float product is exactly 0.5: half to even, bin 0;
        # few enough that rounding up would put them into a bin the 0.1 rule drops), 45 (1.5000001,
        # bin 2), and four near-copy pairs each at 135 and 255 (exactly 4.5 / 8.5: bins 4 / 8),
        # 150 (bin 5) and 350 (bin 12, from a negative difference): four bins tie at 4, below a
        # tenth of the largest.  (No integer difference gives exactly 1.5 or 2.5 in float.)
        rot = rng.choice([3.0, 15.0, 45.0], n, p=[0.66, 0.04, 0.30])
        clean = [i for i in range(300) if knode[part[i]] == 23][:16]
        for j, i in enumerate(clean):
            rot[i] = (135.0, 255.0, 150.0, 350.0)[j // 4]
            k = int(part[i])
            present[k], bad[k] = True, False
            fd[i] = flip_bits(kd[k], j % 3, rng)
        ka[:] = rng.integers(0, 360, n)
        for i in range(300):
            a = fa[i] + rot[i]
            ka[part[i]] = a if a < 360 else a - 360
    else:
        ka[:] = rng.integers(0, 360, n)
    return dict(kd=kd, km=km, kpresent=present, kbad=bad, ka=ka, kfv=csr(knode),
                fd=fd, fm=fm, fa=fa, ffv=csr(fnode))


def scenario_a3(seed, nbytes, th_low):
    """Degenerate: node 7 whose keyframe keypoints all lack map points, node 9 with a single
    frame entry (second-best stays INT_MAX), node 12 ordinary."""
    rng = np.random.default_rng(seed)
    n = 60
    kd = rng.integers(0, 256, (n, nbytes), dtype=np.uint8)
    knode = np.array([7] * 15 + [9] * 5 + [12] * 40)[rng.permutation(n)]
    present = rng.random(n) < 0.9
    present[knode == 7] = False
    present[knode == 9] = True
    bad = np.zeros(n, bool)
    bad[np.flatnonzero(knode == 12)[:3]] = True
    fd = np.stack([flip_bits(kd[i], int(rng.integers(0, 30)), rng) for i in range(n)])
    fnode = knode.copy()
    nine = np.flatnonzero(fnode == 9)
    fnode[nine[1:]] = 12
    return dict(kd=kd, km=None, kpresent=present, kbad=bad, ka=np.zeros(n, np.float32), kfv=csr(knode),
                fd=fd, fm=None, fa=np.zeros(n, np.float32), ffv=csr(fnode))


def scenario_b(seed, nbytes, masked, th_low, n1=300, n2=400):
    rng = np.random.default_rng(seed)
    d1 = rng.integers(0, 256, (n1, nbytes), dtype=np.uint8)
    m1 = rand_masks(rng, n1, nbytes) if masked else None
    m2 = rand_masks(rng, n2, nbytes) if masked else None
    has1, has2 = rng.random(n1) < 0.62, rng.random(n2) < 0.62
    bad1, bad2 = rng.random(n1) < 0.04, rng.random(n2) < 0.04
    special = dict(dup=20, ratio=40, u=60, v=75, th=90)
    d1[special["v"]] = flip_bits(d1[special["u"]], 2, rng)
    part = rng.permutation(n1)                            # KF2 keypoint j < n1 is KF1's part[j]
    d2 = rng.integers(0, 256, (n2, nbytes), dtype=np.uint8)
    for j in range(n1):
        d2[j] = flip_bits(d1[part[j]], int(rng.integers(0, 41 if nbytes >= 32 else 15)), rng)
    p2 = {int(part[j]): j for j in range(n1)}
    extras = list(range(n1, n2))
    ok = lambda a, b: both_set(m1[a], m2[b]) if masked else None  # noqa: E731
    x = special["dup"]
    d2[p2[x]] = d1[x]
    d2[extras[0]] = d1[x]
    if masked:
        m2[extras[0]] = m2[p2[x]]
    y = special["ratio"]
    d2[p2[y]] = flip_bits(d1[y], 10, rng, ok(y, p2[y]))
    d2[extras[1]] = flip_bits(d1[y], 12, rng, ok(y, extras[1]))
    u, v = special["u"], special["v"]
    d2[p2[u]] = flip_bits(d1[u], 1, rng, ok(u, p2[u]))
    d2[p2[v]] = flip_bits(d1[v], 10 if nbytes < 32 else 20, rng, ok(v, p2[v]))
    t = special["th"]
    d2[p2[t]] = flip_bits(d1[t], th_low, rng, ok(t, p2[t]))
    for i in special.values():
        has1[i], bad1[i] = True, False
        has2[p2[i]], bad2[p2[i]] = True, False
    has2[extras[:2]], bad2[extras[:2]] = True, False
    return dict(d1=d1, m1=m1, has1=has1, bad1=bad1, d2=d2, m2=m2, has2=has2, bad2=bad2)


# ------------------------------------------------------------------------------ the cases a run must hold
def classify(log, th_low, nnratio, strict, all_dist):
    """Counts from the reference's own distance records.  all_dist(q) -> {candidate: distance}
    over every candidate the query could have had at the start of the call."""
    c = dict(accepted=0, ratio_rej=0, zero_rej=0, displaced=0, at_th=0)
    taken = set()
    for q, cands in log.queries:
        if not cands:
            continue
        b1 = b2 = INT_MAX
        bi = -1
        for i, d in cands:                      # the update rule of :252-261 / :942-949
            if d < b1:
                b1, b2, bi = d, b1, i
            elif d < b2:
                b2 = d
        under = b1 < th_low if strict else b1 <= th_low
        acc = under and float(b1) < nnratio * float(b2)
        if b1 == th_low and float(b1) < nnratio * float(b2):
            c["at_th"] += 1
        if under and not acc:
            c["ratio_rej"] += 1
            if b1 == 0 and b2 == 0:
                c["zero_rej"] += 1
        if acc:
            c["accepted"] += 1
            full = all_dist(q)
            first = min(full, key=lambda i: (full[i], i))
            if first in taken and first != bi:
                c["displaced"] += 1
            taken.add(bi)
    return c


def require(name, c, keys):
    for k, lo in keys.items():
        if c[k] < lo:
            raise SystemExit("scenario %s lost its %r case: %r" % (name, k, c))
    print("  %s: %s" % (name, c), flush=True)


def np_dist(a, b, ma=None, mb=None):
    x = np.unpackbits(a ^ b)
    if ma is None:
        return int(x.sum())
    return (int((x & np.unpackbits(ma)).sum()) + int((x & np.unpackbits(mb)).sum())) // 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(HERE, "bow_ref.npz"))
    ap.add_argument("--dump", default=None)
    a = ap.parse_args()
    G, log, n_stmt, histo, srcs = load(a.ref)
    if a.dump:
        open(a.dump, "w").write("\n".join(srcs))
    out = {"n_statements": n_stmt, "histo_length": histo}
    nnratio = 0.75

    def matcher(feat_dim, masks, orient):
        Mo = G["Matcher_"]()
        G["f_matcher_ctor"](Mo, nnratio, orient, feat_dim, masks)
        Mo["HISTO_LENGTH"] = histo
        return Mo

    def run_a(name, s, nbytes, masked, orient, keys):
        Mo = matcher(nbytes, masked, orient)
        th = int(Mo["TH_LOW_"])
        kfv, ffv = s["kfv"], s["ffv"]
        K = kf_standin(log, "query", s["kd"], s["km"], s["kpresent"], s["kbad"], s["ka"], make_fv(*kfv))
        F = frame_standin(G, log, s["fd"], s["fm"], s["fa"], make_fv(*ffv))
        vp = rt.Vector(lambda: None)
        log.reset()
        nm = G["f_bow_a"](Mo, rt.Ptr(obj=K), F, vp)
        m = np.full(len(s["fd"]), -1, np.int32)
        for i, p in enumerate(vp.v):
            if p is not None:
                m[i] = p.obj["id"]
        assert int((m >= 0).sum()) == nm
        pre = name + "_"
        out[pre + "kf_desc"], out[pre + "f_desc"] = s["kd"], s["fd"]
        if masked:
            out[pre + "kf_mask"], out[pre + "f_mask"] = s["km"], s["fm"]
        out[pre + "kf_angle"], out[pre + "f_angle"] = s["ka"], s["fa"]
        out[pre + "kf_has"] = (s["kpresent"] & ~s["kbad"]).astype(np.uint8)
        for tag, fv in (("kf", kfv), ("f", ffv)):
            out[pre + tag + "_fv_node"], out[pre + tag + "_fv_ptr"], out[pre + tag + "_fv_feat"] = fv
        out[pre + "meta"] = np.array([nbytes, int(masked), int(orient), th], np.int32)
        out[pre + "nnratio"] = nnratio
        out[pre + "match_f"], out[pre + "nmatches"] = m, nm
        fnode = {int(nd): [int(x) for x in ffv[2][ffv[1][j]:ffv[1][j + 1]]] for j, nd in enumerate(ffv[0])}
        node_of = {}
        for j, nd in enumerate(kfv[0]):
            for x in kfv[2][kfv[1][j]:kfv[1][j + 1]]:
                node_of[int(x)] = int(nd)

        def all_dist(q):
            return {i: np_dist(s["kd"][q], s["fd"][i], s["km"][q] if masked else None,
                               s["fm"][i] if masked else None) for i in fnode.get(node_of[q], [])}
        c = classify(log, th, nnratio, False, all_dist)
        c["removed"] = c["accepted"] - nm
        if orient:
            sizes, inds = log.maxima
            nz = sorted(x for x in sizes if x > 0)
            c["half"] = sum(1 for x, _ in log.rounds if x - np.floor(x) == 0.5)
            c["negative_rot"] = sum(1 for x, r in log.rounds if r >= 11)
            c["bin_tie"] = int(len(nz) != len(set(nz)))
            c["third_dropped"] = int(inds[2] == -1 and inds[1] != -1 and len(nz) >= 3)
            out[pre + "hist"] = np.array(sizes, np.int32)
            out[pre + "maxima"] = np.array(inds, np.int32)
        require(name, c, keys)
        return nm

    full = dict(accepted=30, ratio_rej=1, zero_rej=1, displaced=1, at_th=1)
    run_a("a0", scenario_a(101, 32, False, 64, False), 32, False, False, full)
    run_a("a1", scenario_a(102, 32, True, 32, False), 32, True, False, full)
    run_a("a2", scenario_a(103, 32, False, 64, True), 32, False, True,
          dict(full, removed=1, half=3, negative_rot=1, bin_tie=1, third_dropped=1))
    s3 = scenario_a3(104, 32, 64)
    run_a("a3", s3, 32, False, False, dict(accepted=3))
    empty = (np.zeros(0, np.uint32), np.zeros(1, np.int32), np.zeros(0, np.uint32))
    assert run_a("a3k", dict(s3, kfv=empty), 32, False, False, {}) == 0
    assert run_a("a3f", dict(s3, ffv=empty), 32, False, False, {}) == 0

    def run_b(name, s, nbytes, masked):
        Mo = matcher(nbytes, masked, False)
        th = int(Mo["TH_LOW_"])
        K1 = kf_standin(log, "query", s["d1"], s["m1"], s["has1"], s["bad1"])
        K2 = kf_standin(log, "cand", s["d2"], s["m2"], s["has2"], s["bad2"])
        vp = rt.Vector(lambda: None)
        log.reset()
        nm = G["f_bow_b"](Mo, rt.Ptr(obj=K1), rt.Ptr(obj=K2), vp)
        m = np.full(len(s["d1"]), -1, np.int32)
        for i, p in enumerate(vp.v):
            if p is not None:
                m[i] = p.obj["id"]
        assert int((m >= 0).sum()) == nm
        pre = name + "_"
        out[pre + "desc1"], out[pre + "desc2"] = s["d1"], s["d2"]
        if masked:
            out[pre + "mask1"], out[pre + "mask2"] = s["m1"], s["m2"]
        good2 = s["has2"] & ~s["bad2"]
        out[pre + "has1"] = (s["has1"] & ~s["bad1"]).astype(np.uint8)
        out[pre + "has2"] = good2.astype(np.uint8)
        out[pre + "meta"] = np.array([nbytes, int(masked), 0, th], np.int32)
        out[pre + "nnratio"] = nnratio
        out[pre + "matches12"], out[pre + "nmatches"] = m, nm

        def all_dist(q):
            return {int(i): np_dist(s["d1"][q], s["d2"][i], s["m1"][q] if masked else None,
                                    s["m2"][i] if masked else None) for i in np.flatnonzero(good2)}
        c = classify(log, th, nnratio, True, all_dist)
        assert c["accepted"] == nm
        require(name, c, dict(accepted=30, ratio_rej=1, zero_rej=1, displaced=1, at_th=1))

    run_b("b0", scenario_b(201, 32, False, 64), 32, False)
    run_b("b1", scenario_b(202, 16, True, 16), 16, True)
    run_b("b2", scenario_b(203, 64, False, 128), 64, False)
    np.savez_compressed(a.out, **out)
    print("wrote %s (%d statements translated)" % (a.out, n_stmt))


if __name__ == "__main__":
    main()
