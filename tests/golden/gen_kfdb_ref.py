"""Generate tests/golden/kfdb_ref.npz: the keyframe database queries, evaluated from the reference
TEXT on scripted keyframes (no reference source is stored: the fixture holds numbers only).

Translated from the reference checkout by tests/golden/cxx_eval.py (safe_exec runs the result with
no builtins; cxx_eval / cxx_rt / safe_exec are imported unchanged):
  cMultiKeyFrameDatabase::add / erase                 src/cMultiKeyFrameDatabase.cpp:43-73
  cMultiKeyFrameDatabase::DetectLoopCandidates        :82-221
  cMultiKeyFrameDatabase::DetectRelocalisationCandidates   :223-340
  L1Scoring::score                                    ThirdParty/DBoW2/DBoW2/ScoringObject.cpp:23-68
  the minScore loop of cLoopClosing::DetectLoop       src/cLoopClosing.cpp:141-157, as it stands in
      the function body (its locals become parameters: vpConnectedKeyFrames, CurrentBowVec; its
      result minScore is returned)
Stand-ins, registered here:
  * std::set<cMultiKeyFrame*> (count, insert) is not in the translator's runtime: RefSet below;
  * DBoW2::BowVector is `class BowVector : public std::map<WordId, WordValue>`: the names are
    expanded to that map type by the translator's macro table, and std::map::lower_bound (used by
    L1Scoring::score) is supplied as gen_bow_ref.py supplies it;
  * `std::unique_lock<std::mutex> lock(mMutex);` is dropped (one thread);
  * mpVoc->score / mpORBVocabulary->score call the translated L1Scoring::score (the Lafida
    vocabulary's scoringType 0);
  * cMultiKeyFrame / cMultiFrame are scripted objects holding mnId, mBowVec, the connected set, the
    neighbour list and the six members mnLoopQuery ... mRelocScore.
The scenarios are tests/kfdb_cases.py's.  main() asserts from its records that every case the tests
are about really occurs in the reference's run, so the fixture cannot go trivial.

    python tests/golden/gen_kfdb_ref.py [--ref /root/reference] [--out tests/golden/kfdb_ref.npz]
"""
import argparse
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import cxx_eval  # noqa: E402
import cxx_rt as rt  # noqa: E402
from cxx_eval import (BOOL, DOUBLE, INT, VOID, ClassSpec, Cls, Ctx, E, Fn, PtrT, Unsupported,  # noqa: E402
                      build_env, translate_function)
from safe_exec import safe_exec  # noqa: E402

V = lambda t: Cls("vector", (t,))  # noqa: E731
c_ref = lambda t: (t, True, True)  # noqa: E731
val = lambda t: (t, False, True)  # noqa: E731
MKF, MF, VOC = Cls("cMultiKeyFrame"), Cls("cMultiFrame"), Cls("ORBVocabulary")
BOW = Cls("map", (INT, DOUBLE))
SET = Cls("set", (PtrT(MKF),))
MEMBERS = ("mnLoopQuery", "mnLoopWords", "mLoopScore", "mnRelocQuery", "mnRelocWords", "mRelocScore")
NAMES = ("loop_query", "loop_words", "loop_score", "reloc_query", "reloc_words", "reloc_score")


def _sig(params, ret):
    return Fn(None, params, ret)


class RefSet:
    """std::set<cMultiKeyFrame*>: count and insert (pointers compare by the object they name)."""

    def __init__(self, items=()):
        self.s = set(items)

    def __getitem__(self, k):
        return {"count": lambda p: 1 if p in self.s else 0, "insert": self.s.add}[k]

    def copy(self):
        return RefSet(self.s)


class BowMap(rt.Map):
    """std::map<WordId, WordValue> with lower_bound."""
    __slots__ = ()

    def __init__(self, fac=None):
        rt.Map.__init__(self, fac or (lambda: 0.0), ordered=True)

    def copy(self):
        m = BowMap(self.fac)
        m.d = dict(self.d)
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


def find_fn(src, pattern):
    m = re.search(pattern, src)
    if not m:
        raise Unsupported("no definition matching %r" % pattern)
    return cxx_eval.find_function(src, src[m.start():m.end()])


def load(ref):
    rd = lambda *p: open(os.path.join(ref, *p), encoding="latin-1").read()  # noqa: E731
    db_cpp = rd("src", "cMultiKeyFrameDatabase.cpp")
    sc_cpp = rd("ThirdParty", "DBoW2", "DBoW2", "ScoringObject.cpp")
    lc_cpp = rd("src", "cLoopClosing.cpp")
    cxx_eval.FuncTranslator.method_call = _method_call
    ctx = Ctx()
    macros = {"DBoW2": (None, cxx_eval.tokenize("std")),
              "BowVector": (None, cxx_eval.tokenize("map<unsigned int, double>")),
              "WordValue": (None, cxx_eval.tokenize("double"))}
    ctx.add_class(ClassSpec("set", {}, {"count": _sig([val(PtrT(MKF))], INT), "insert": _sig([val(PtrT(MKF))], VOID)},
                            ctor="Set_", runtime_ctor=RefSet))
    ctx.add_class(ClassSpec("ORBVocabulary", {}, {"score": Fn("f_score_m", [c_ref(BOW), c_ref(BOW)], DOUBLE)}))
    ctx.add_class(ClassSpec("cMultiKeyFrame", {
        "mnId": INT, "mBowVec": BOW, "mnLoopQuery": INT, "mnLoopWords": INT, "mLoopScore": DOUBLE,
        "mnRelocQuery": INT, "mnRelocWords": INT, "mRelocScore": DOUBLE}, {
        "GetConnectedKeyFrames": _sig([], SET), "GetBestCovisibilityKeyFrames": _sig([c_ref(INT)], V(PtrT(MKF))),
        "isBad": _sig([], BOOL), "GetBowVector": _sig([], BOW)}))
    ctx.add_class(ClassSpec("cMultiFrame", {"mnId": INT, "mBowVec": BOW}))
    dbc = ClassSpec("cMultiKeyFrameDatabase", {"mvInvertedFile": V(Cls("list", (PtrT(MKF),))), "mpVoc": PtrT(VOC)},
                    ctor="Database_")
    ctx.add_class(dbc)
    lcc = ClassSpec("cLoopClosing", {"mpORBVocabulary": PtrT(VOC)}, ctor="LoopClosing_")
    ctx.add_class(lcc)
    ctx.add_class(ClassSpec("L1Scoring", {}, ctor="L1Scoring_"))
    ctx.funcs["make_pair"] = Fn("_Pair", None, lambda ts: Cls("pair", tuple(ts)))
    ctx.funcs["fabs"] = Fn("s_fabs", [val(DOUBLE)], DOUBLE)
    srcs, n_stmt = [], [0]
    unlock = lambda body: re.sub(r"(std::)?unique_lock\s*<\s*(std::)?mutex\s*>\s*lock\s*\(\s*mMutex\s*\)\s*;", "", body)  # noqa: E731

    def fn(pyname, src, pattern, this=None, ret=VOID, params=None, body=None):
        p, _, b = find_fn(src, pattern)
        b = unlock(b if body is None else body(b))
        n_stmt[0] += b.count(";")
        srcs.append(translate_function(ctx, pyname, p if params is None else params, b, this_cls=this, ret=ret,
                                       macros=macros))
    # parameter lists are parsed without the macro table: BowVector is spelled out there
    bow_t = "std::map<unsigned int, double>"
    fn("f_score", sc_cpp, r"double L1Scoring::score\(", this=ctx.classes["L1Scoring"], ret=DOUBLE,
       params="const %s &v1, const %s &v2" % (bow_t, bow_t))
    fn("f_add", db_cpp, r"void cMultiKeyFrameDatabase::add\(", this=dbc)
    fn("f_erase", db_cpp, r"void cMultiKeyFrameDatabase::erase\(", this=dbc)
    fn("f_loop", db_cpp, r"vector<cMultiKeyFrame\*> cMultiKeyFrameDatabase::DetectLoopCandidates\(", this=dbc,
       ret=V(PtrT(MKF)))
    fn("f_reloc", db_cpp, r"std::vector<cMultiKeyFrame\*> cMultiKeyFrameDatabase::DetectRelocalisationCandidates\(",
       this=dbc, ret=V(PtrT(MKF)))

    def min_loop(body):
        """The minScore loop out of DetectLoop's body: from `double minScore = 1;` to the loop's end."""
        m = re.search(r"double\s+minScore\s*=\s*1(\.0)?\s*;", body)
        if not m:
            raise Unsupported("no minScore loop in DetectLoop")
        i = body.index("{", body.index("for", m.end()))
        depth, j = 0, i
        while True:
            depth += {"{": 1, "}": -1}.get(body[j], 0)
            j += 1
            if depth == 0:
                break
        return body[m.start():j] + "\nreturn minScore;\n"
    fn("f_min", lc_cpp, r"bool cLoopClosing::DetectLoop\(", this=lcc, ret=DOUBLE, body=min_loop,
       params="const std::vector<cMultiKeyFrame*>& vpConnectedKeyFrames, const %s& CurrentBowVec" % bow_t)
    env = build_env(ctx, rt, {"s_fabs": abs})
    G = safe_exec("\n".join(srcs), env, "<ref:cMultiKeyFrameDatabase.cpp>")
    l1 = rt.Struct("L1Scoring", {})
    env["f_score_m"] = G["f_score_m"] = lambda voc, a, b: G["f_score"](l1, a, b)
    return G, n_stmt[0]


def bow_map(word, value):
    m = BowMap()
    for w, v in zip(np.asarray(word).tolist(), np.asarray(value, np.float64).tolist()):
        m.d[int(w)] = float(v)
    return m


class RefDB:
    """tests/np_kfdb.Database's interface on the translated text."""

    def __init__(self, G, n_words):
        self.G = G
        voc = rt.Ptr(obj=rt.Struct("ORBVocabulary", {}))
        self.db = rt.Struct("cMultiKeyFrameDatabase", {
            "mvInvertedFile": rt.Vector(lambda: rt.List(lambda: None), [rt.List(lambda: None) for _ in range(n_words)]),
            "mpVoc": voc})
        self.lc = rt.Struct("cLoopClosing", {"mpORBVocabulary": voc})
        self.kfs, self.ptrs, self.alive = [], [], []
        self.connected, self.neigh = RefSet(), None

    def _kf(self, slot, word, value, score_init):
        f = {"mnId": 0, "mBowVec": bow_map(word, value), "mnLoopQuery": 0, "mnLoopWords": 0,
             "mLoopScore": float(score_init), "mnRelocQuery": 0, "mnRelocWords": 0, "mRelocScore": float(score_init),
             "isBad": lambda: False}
        f["GetBowVector"] = lambda: f["mBowVec"]
        f["GetConnectedKeyFrames"] = lambda: self.connected
        f["GetBestCovisibilityKeyFrames"] = lambda n: rt.Vector(
            lambda: None, [self.ptrs[s] for s in np.asarray(self.neigh[slot]).tolist()[:n] if 0 <= s < len(self.ptrs)])
        return rt.Struct("cMultiKeyFrame", f)

    def add(self, word, value, reloc_score_init=0.0):
        kf = self._kf(len(self.kfs), word, value, reloc_score_init)
        self.kfs.append(kf)
        self.ptrs.append(rt.Ptr(obj=kf))
        self.alive.append(True)
        self.G["f_add"](self.db, self.ptrs[-1])
        return len(self.kfs) - 1

    def erase(self, slot):
        self.alive[slot] = False
        self.G["f_erase"](self.db, self.ptrs[slot])

    def members(self):
        dts = (np.int64, np.int32, np.float64) * 2
        return {n: np.array([kf[m] for kf in self.kfs], dt) for n, m, dt in zip(NAMES, MEMBERS, dts)}

    def min_score(self, qw, qv, slots):
        vp = rt.Vector(lambda: None, [self.ptrs[s] for s in slots if 0 <= s < len(self.ptrs)])
        return float(self.G["f_min"](self.lc, vp, bow_map(qw, qv)))

    def _diag(self, qw, qv):
        """Per slot: the words an alive keyframe shares with the query and the text's score of it."""
        q, qs = bow_map(qw, qv), set(np.asarray(qw).tolist())
        common, score = np.zeros(len(self.kfs), np.int32), np.zeros(len(self.kfs))
        for s, kf in enumerate(self.kfs):
            if self.alive[s]:
                common[s] = sum(1 for w in kf["mBowVec"].d if w in qs)
                score[s] = self.G["f_score_m"](None, q, kf["mBowVec"])
            else:
                score[s] = -0.0
        return common, score

    def _slots(self, vec):
        out = []
        for i in range(vec.m_size()):
            p = vec[i]
            out.append(next(s for s, q in enumerate(self.ptrs) if q == p))
        return out

    def detect_loop(self, qw, qv, query_id, connected, min_score, neigh):
        common, score = self._diag(qw, qv)
        self.connected = RefSet(self.ptrs[s] for s in np.flatnonzero(np.asarray(connected)).tolist())
        self.neigh = neigh
        q = self._kf(-1, qw, qv, 0.0)
        q["mnId"] = int(query_id)
        r = self.G["f_loop"](self.db, rt.Ptr(obj=q), float(min_score))
        return {"candidates": self._slots(r), "common": common, "score": score}

    def detect_reloc(self, qw, qv, query_id, neigh):
        common, score = self._diag(qw, qv)
        self.neigh = neigh
        f = rt.Struct("cMultiFrame", {"mnId": int(query_id), "mBowVec": bow_map(qw, qv)})
        r = self.G["f_reloc"](self.db, rt.Ptr(obj=f))
        return {"candidates": self._slots(r), "common": common, "score": score}


def require(recs):
    """Every case the tests are about occurs in the reference's own run."""
    def rec(name, kind, nth=0):
        return [r for r in recs[name] if r["kind"] == kind][nth]
    for kind in ("reloc", "loop"):
        r = rec("retain_exact", kind)
        assert r["score"][0] == 0.75 * r["score"][1] and r["candidates"].tolist() == [1, 2]      # strict >
    assert rec("min_score_equal", "min")["min_score"] == rec("min_score_equal", "loop")["score"][0]
    assert rec("min_score_equal", "loop")["candidates"].tolist() == [0, 2]                        # >=
    assert rec("dedupe", "reloc")["candidates"].tolist() == [3, 1] == rec("dedupe", "loop")["candidates"].tolist()
    r1, r2 = rec("stale_reloc", "reloc", 0), rec("stale_reloc", "reloc", 1)
    assert r2["reloc_score"][2] == r1["reloc_score"][2] != r2["score"][2] and r2["candidates"].tolist() == [0]
    assert r2["score"][1] > 0.75 * r2["score"][0]
    r = rec("connected", "loop")
    assert r["loop_words"][1] == 1 and r["loop_words"][3] == 1 and r["common"][1] > 1 and r["loop_query"][1] == 0
    assert len(rec("random65", "loop", 0)["candidates"]) == 0 and rec("random65", "loop", 0)["common"].max() > 0
    assert len(rec("random65", "loop", 1)["candidates"]) > 0 and len(rec("random65", "loop", 2)["candidates"]) == 0
    r = rec("random301", "reloc", 1)
    assert r["common"][150] == 0 and r["common"][100] == 0 and len(r["candidates"]) > 1
    assert rec("lengths", "loop")["common"].tolist() == [0, 1, 2, 2, 3, 4, 0]
    assert len(rec("lengths", "reloc", 2)["candidates"]) == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(HERE, "kfdb_ref.npz"))
    a = ap.parse_args()
    from tests import kfdb_cases as kc
    G, n_stmt = load(a.ref)
    out, recs = {}, {}
    for case in kc.all_cases():
        recs[case["name"]] = r = kc.run(RefDB(G, case["n_words"]), case)
        out[case["name"] + "/kinds"] = np.array([("min", "loop", "reloc").index(x["kind"]) for x in r], np.int32)
        for i, x in enumerate(r):
            for k, v in x.items():
                if k != "kind":
                    out["%s/%d/%s" % (case["name"], i, k)] = np.asarray(v)
    require(recs)
    np.savez_compressed(a.out, **out)
    print("wrote %s: %d scenarios, %d records, %d reference statements translated, %d bytes"
          % (a.out, len(recs), sum(len(r) for r in recs.values()), n_stmt, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
