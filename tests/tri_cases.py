"""Inputs for the device SearchForTriangulationRaw (csrc/tri_search.hip) that reach each of its
paths, and a numpy restatement of its control flow that says which paths an input reaches.

build() makes a keyframe pair in which every row is a random descriptor (random pairs sit about
4 * nbytes bits apart, never within TH_LOW) except the rows that *clusters* override with noisy
copies of one base descriptor: which query lists which KF2 row, in which train segment and at
which distance is then exact.  paths() restates the pipeline's decisions only -- per (query,
segment) counts, the overflow flag, the private / flagged split, the key offsets and the branch
the ordered pass takes per flagged query -- and returns the matches that decomposition yields.
The constants below are copies of the kernels'; tests/test_tri_paths.py holds them to the
sources, so retuning one invalidates the path table loudly.
"""
import collections
import functools
import types

import numpy as np

# csrc/tri_search.hip (kTriSeg, kTriSub, kTriWin) and csrc/ham_dist.hpp (kHamTile)
K_TRI_SEG, K_TRI_SUB, K_TRI_WIN, K_HAM_TILE = 16, 96, 1024, 256

# every path paths() can report; tests/test_tri_paths.py asserts the case table covers them all
ALL_PATHS = (
    "radius_one_tile", "radius_multi_tile", "radius_partial_tile", "radius_empty_segments",
    "slot_overflow_pairs", "global_overflow",
    "q_empty", "q_private_won", "q_private_nomatch", "q_flagged", "q_slot_over", "q_cap_over_only",
    "private_and_ordered_in_one_call",
    "ns_0", "ns_64", "ns_65", "entry_chunks_multi",
    "ens_first", "ens_same", "ens_next", "ens_jump",
    "seq_pair", "seq_pair_second_sees_first_winner", "seq_pair_straddles_window",
    "seq_pair_refused_span", "seq_one_round", "seq_multi_round", "seq_single_straddles_window",
    "seq_multi_best_in_later_round", "seq_multi_winner_after_best_round",
    "seq_multi_early_break", "seq_multi_last_key_at_threshold", "seq_multi_all_taken",
    "seq_rescan", "seq_rescan_won", "seq_nearest_already_taken", "lds_over_64k", "ncams_1",
)


def descs(n, nbytes=32, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, nbytes), dtype=np.uint8)


def noisy(d, nflip, seed):
    """Copies of the rows of d with exactly nflip[i] distinct bits flipped."""
    rng = np.random.default_rng(seed)
    bits = np.unpackbits(d, axis=1)
    for i in range(len(bits)):
        bits[i, rng.choice(bits.shape[1], int(nflip[i]), replace=False)] ^= 1
    return np.packbits(bits, axis=1)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def epi_dsqr(r1, r2, Em):
    """CheckDistEpipolarLine's (nom^2 / den) in float64 for ray r1 against rows r2 (NaN: den == 0)."""
    r2 = np.atleast_2d(r2)
    nom = (r2 @ Em) @ r1
    ex1 = Em @ r1
    etx2 = r2 @ Em
    den = ex1 @ ex1 + (etx2 * etx2).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den == 0.0, np.nan, nom * nom / den)


def _dists(q, qm, t, tm):
    """DescriptorDistance64 / ...Masked of one query row against rows t."""
    x = (q[None, :] ^ t).view(np.uint64)
    if qm is None:
        return np.bitwise_count(x).sum(1).astype(np.int64)
    s = np.bitwise_count(x & qm.view(np.uint64)[None, :]).sum(1).astype(np.int64)
    s += np.bitwise_count(x & tm.view(np.uint64)).sum(1).astype(np.int64)
    return s // 2


def _candidates(case):
    """Per query the rows within TH_LOW: arrays (idx2 ascending, dist)."""
    by_cam = [np.nonzero((case.cam2 == c) & (case.has2 == 0))[0] for c in range(case.ncams)]
    out = []
    for q in range(len(case.d1)):
        rows = by_cam[case.cam1[q]] if not case.has1[q] else np.zeros(0, np.int64)
        if len(rows) == 0:
            out.append((np.zeros(0, np.int64), np.zeros(0, np.int64)))
            continue
        d = _dists(case.d1[q], None if case.m1 is None else case.m1[q], case.d2[rows],
                   None if case.m2 is None else case.m2[rows])
        sel = d <= case.th_low
        out.append((rows[sel], d[sel]))
    return out


def _make(n1, n2, ncams, clusters, nbytes, masked, seed, thresh):
    rng = np.random.default_rng(seed)
    d1 = descs(n1, nbytes, seed + 1)
    d2 = descs(n2, nbytes, seed + 2)
    cam1 = rng.integers(0, ncams, n1).astype(np.int32)
    cam2 = rng.integers(0, ncams, n2).astype(np.int32)
    r1 = _unit(rng.normal(size=(n1, 3)))
    r2 = _unit(rng.normal(size=(n2, 3)))
    E = rng.normal(size=(ncams, ncams, 3, 3))
    bases = descs(max(1, len(clusters)), nbytes, seed + 3)
    for k, c in enumerate(clusters):
        q = np.asarray(c["q"], np.int64)
        t = np.asarray(c["t"], np.int64)
        qf = c["qflips"] if "qflips" in c else rng.integers(*c.get("qflip", (0, 1)), len(q))
        tf = c["tflips"] if "tflips" in c else rng.integers(*c["tflip"], len(t))
        d1[q] = noisy(np.repeat(bases[k:k + 1], len(q), 0), qf, seed + 10 + k)
        d2[t] = noisy(np.repeat(bases[k:k + 1], len(t), 0), tf, seed + 5000 + k)
        cam1[q] = c["cam"]
        cam2[t] = c["cam"]
        if "passes" in c:
            # the cluster's queries share one ray; a row in `passes` lies on its epipolar plane
            # (nom ~ 0), every other row of the cluster along E r1 (nom^2 / den of order 1)
            ray = _unit(rng.normal(size=3))
            r1[q] = ray
            u = E[c["cam"], c["cam"]] @ ray
            ok = set(int(x) for x in c["passes"])
            for row in t:
                r2[row] = _unit(np.cross(u, rng.normal(size=3))) if int(row) in ok else _unit(u)
        for row, qq in c.get("pass_for", {}).items():
            # the row lies on the epipolar plane of that one query's own ray
            r2[row] = _unit(np.cross(E[c["cam"], c["cam"]] @ r1[qq], rng.normal(size=3)))
    case = types.SimpleNamespace(
        d1=d1, d2=d2, m1=None, m2=None, cam1=cam1, cam2=cam2, has1=np.zeros(n1, np.uint8),
        has2=np.zeros(n2, np.uint8), r1=np.ascontiguousarray(r1), r2=np.ascontiguousarray(r2),
        E=np.ascontiguousarray(E), ncams=ncams, nbytes=nbytes, masked=masked,
        th_low=nbytes if masked else 2 * nbytes, thresh=thresh, seed=seed)
    if masked:
        keep = np.random.default_rng(seed + 7).random((n1 + n2, nbytes * 8)) < 0.9
        m = np.packbits(keep.astype(np.uint8), axis=1)
        case.m1, case.m2 = np.ascontiguousarray(m[:n1]), np.ascontiguousarray(m[n1:])
    return case


def _verdict_margin_ok(case):
    """No candidate's nom^2 / den within 1e-9 relative of thresh: no verdict turns on rounding."""
    for q, (rows, _) in enumerate(_candidates(case)):
        if len(rows) == 0:
            continue
        c = case.cam1[q]
        v = epi_dsqr(case.r1[q], case.r2[rows], case.E[c, c])
        if np.any(np.abs(v[~np.isnan(v)] - case.thresh) <= 1e-9 * abs(case.thresh)):
            return False
    return True


def build(n1, n2, ncams, clusters, nbytes=32, masked=False, seed=0, thresh=1e9):
    """clusters: dicts with cam, q (KF1 rows), t (KF2 rows), flip-count ranges qflip / tflip
    (half-open, default no query flips) or explicit per-row counts qflips / tflips, and optionally
    passes (the rows of t that pass the epipolar check for the cluster's queries; the others
    fail) or pass_for (row -> the one query it is made to pass with).  TH_LOW is the reference's:
    2 * nbytes, nbytes with masks.  Moves to the next seed while any candidate's epipolar value
    lies within 1e-9 relative of thresh."""
    for s in range(seed, seed + 16):
        case = _make(n1, n2, ncams, clusters, nbytes, masked, s, thresh)
        if _verdict_margin_ok(case):
            return case
    raise AssertionError("no seed with every epipolar verdict clear of the threshold")


def from_arrays(d1, d2, cam1, cam2, has1, has2, r1, r2, E, thresh, m1=None, m2=None):
    """A case from the arrays the older fixtures of tests/test_matcher.py return."""
    nbytes = d1.shape[1]
    return types.SimpleNamespace(
        d1=d1, d2=d2, m1=m1, m2=m2, cam1=cam1, cam2=cam2, has1=has1, has2=has2,
        r1=np.ascontiguousarray(r1), r2=np.ascontiguousarray(r2), E=np.ascontiguousarray(E),
        ncams=E.shape[0], nbytes=nbytes, masked=m1 is not None,
        th_low=nbytes if m1 is not None else 2 * nbytes, thresh=thresh, seed=None)


def tri_lds_bytes(n2, ncams):
    return ncams * 2 * K_TRI_WIN * 4 + ((((n2 + 31) // 32) + 3) & ~3) * 4


def paths(case):
    """(Counter of paths reached, matches12 the decomposition yields)."""
    n1, n2, ncams = len(case.d1), len(case.d2), case.ncams
    SEG, SUB, WIN, TILE = K_TRI_SEG, K_TRI_SUB, K_TRI_WIN, K_HAM_TILE
    P = collections.Counter()
    # k_tri_radius: the train rows in SEG segments of `per` rows, each walked in tiles
    per = -(-(-(-n2 // SEG)) // TILE) * TILE
    seg_rows = [min(n2, (s + 1) * per) - s * per for s in range(SEG) if s * per < n2]
    P["tiles_per_seg_max"] = max(-(-r // TILE) for r in seg_rows)
    P["segs_nonempty"] = len(seg_rows)
    P["radius_one_tile"] = sum(1 for r in seg_rows if r <= TILE)
    P["radius_multi_tile"] = sum(1 for r in seg_rows if r > TILE)
    P["radius_partial_tile"] = sum(1 for r in seg_rows if r % TILE)
    P["radius_empty_segments"] = SEG - len(seg_rows)
    lds = tri_lds_bytes(n2, ncams)
    P["lds_bytes"] = lds
    P["lds_over_64k"] = int(lds > 64 * 1024)
    P["ncams_1"] = int(ncams == 1)
    cands = _candidates(case)
    segcnt = np.zeros((n1, SEG), np.int64)
    ref_all = np.zeros(n2, np.int64)
    ref_pass = np.zeros(n2, np.int64)
    keys = []          # per query: (dist, idx2, passes) ascending -- the gathered key order
    for q, (rows, d) in enumerate(cands):
        if len(rows) == 0:
            keys.append([])
            continue
        c = case.cam1[q]
        v = epi_dsqr(case.r1[q], case.r2[rows], case.E[c, c])
        ok = v < case.thresh          # NaN (den == 0) compares false
        np.add.at(segcnt[q], rows // per, 1)
        ref_all[rows] += 1
        # k_tri_pass sees the stored candidates only: the first SUB of a segment in row order
        rank = np.zeros(len(rows), np.int64)
        for s in np.unique(rows // per):
            m = rows // per == s
            rank[m] = np.arange(int(m.sum()))
        ref_pass[rows[(rank < SUB) & ok]] += 1
        keys.append(sorted(zip(d.tolist(), rows.tolist(), ok.tolist())))
    slot_over = segcnt > SUB
    gover = bool(slot_over.any())
    P["slot_overflow_pairs"] = int(slot_over.sum())
    P["global_overflow"] = int(gover)
    # k_tri_private
    m = -np.ones(n1, np.int64)
    flagged = []       # (query, len): len 0 means rescan
    for q in range(n1):
        c = len(keys[q])
        if slot_over[q].any():
            P["q_slot_over"] += 1
            flagged.append((q, 0))
            continue
        if c > WIN:
            P["q_cap_over_only"] += 1
            flagged.append((q, 0))
            continue
        if c == 0:
            P["q_empty"] += 1
            continue
        by_all = any(p and ref_all[i2] > 1 for _, i2, p in keys[q])
        by_pass = any(ref_pass[i2] - int(p) > 0 for _, i2, p in keys[q])
        if gover or by_all or by_pass:
            P["q_flagged"] += 1
            flagged.append((q, c))
            continue
        th = 2 * keys[q][0][0]
        w = [k for k in keys[q] if k[2] and k[0] <= th]
        if w:
            m[q] = w[0][1]
            P["q_private_won"] += 1
        else:
            P["q_private_nomatch"] += 1
    P["private_and_ordered_in_one_call"] = int(
        not gover and P["q_private_won"] + P["q_private_nomatch"] > 0 and P["q_flagged"] > 0)
    ns = len(flagged)
    P["ns"] = ns
    for v in (0, 64, 65):
        P["ns_%d" % v] = int(ns == v)
    P["cams_with_flagged"] = len({int(case.cam1[q]) for q, _ in flagged})
    P["entry_chunks"] = -(-ns // 64)
    P["entry_chunks_multi"] = int(ns > 64)
    koff = np.concatenate([[0], np.cumsum([c for _, c in flagged])]).astype(np.int64)
    P["flat_keys"] = int(koff[-1])
    # k_tri_seq: one wave per camera over the flagged list in chunks of 64 entries
    matched = np.zeros(n2, bool)

    def first_round(ks):
        """One ballot pair over <= 64 keys (or 32 per half): best, then the winner."""
        un = [k for k in ks if not matched[k[1]]]
        if not un:
            return -1
        th = 2 * un[0][0]
        for d, i2, p in un:
            if p and d <= th:
                return i2
        return -1

    def rescan(q):
        un = [k for k in keys[q] if not matched[k[1]]]
        if not un:
            return -1
        th = 2 * un[0][0]
        for d, i2, p in un:
            if d <= th and p:
                return i2
        return -1

    def multi_round(q):
        ks = keys[q]
        c = len(ks)
        un = [t for t in range(c) if not matched[ks[t][1]]]
        if not un:
            P["seq_multi_all_taken"] += 1
            return -1
        rb = un[0] // 64
        P["seq_multi_best_in_later_round"] += int(rb > 0)
        th = 2 * ks[un[0]][0]
        at_th = False
        for r in range(rb, -(-c // 64)):
            chunk = ks[r * 64:(r + 1) * 64]
            for d, i2, p in chunk:
                if p and d <= th and not matched[i2]:
                    P["seq_multi_winner_after_best_round"] += int(r > rb)
                    P["seq_multi_last_key_at_threshold"] += int(at_th)
                    return i2
            last = chunk[63][0] if len(chunk) == 64 else 1023   # an invalid lane reads all ones
            if last > th:
                P["seq_multi_early_break"] += int((r + 1) * 64 < c)
                return -1
            at_th = at_th or last == th
        return -1

    for cam in range(ncams):
        cw = [-8]

        def ensure(o):
            w0 = int(o) // WIN
            if w0 == cw[0]:
                P["ens_same"] += 1
            elif w0 == cw[0] + 1:
                P["ens_next"] += 1
                cw[0] += 1
            else:
                P["ens_first" if cw[0] == -8 else "ens_jump"] += 1
                cw[0] = w0

        for base in range(0, ns, 64):
            todo = [i for i in range(base, min(ns, base + 64)) if case.cam1[flagged[i][0]] == cam]
            while todo:
                i = todo.pop(0)
                q, c = flagged[i]
                o = int(koff[i])
                if todo and 0 < c <= 32:
                    q2, c2 = flagged[todo[0]]
                    o2 = int(koff[todo[0]])
                    if 0 < c2 <= 32:
                        if o2 + c2 - o <= WIN:
                            todo.pop(0)
                            ensure(o)
                            P["seq_pair"] += 1
                            P["seq_pair_straddles_window"] += int(o // WIN != (o2 + c2 - 1) // WIN)
                            P["seq_nearest_already_taken"] += int(matched[keys[q][0][1]])
                            a = first_round(keys[q])
                            if a >= 0 and any(k[1] == a for k in keys[q2]):
                                P["seq_pair_second_sees_first_winner"] += 1
                            P["seq_nearest_already_taken"] += int(matched[keys[q2][0][1]] or keys[q2][0][1] == a)
                            b = first_round([k for k in keys[q2] if k[1] != a])
                            m[q], m[q2] = a, b
                            if a >= 0:
                                matched[a] = True
                            if b >= 0:
                                matched[b] = True
                            continue
                        P["seq_pair_refused_span"] += 1
                if c > 0:
                    P["seq_nearest_already_taken"] += int(matched[keys[q][0][1]])
                    ensure(o)
                    P["seq_single_straddles_window"] += int(o // WIN != (o + c - 1) // WIN)
                    if c <= 64:
                        P["seq_one_round"] += 1
                        r = first_round(keys[q])
                    else:
                        P["seq_multi_round"] += 1
                        r = multi_round(q)
                else:
                    P["seq_rescan"] += 1
                    r = rescan(q)
                    P["seq_rescan_won"] += int(r >= 0)
                m[q] = r
                if r >= 0:
                    matched[r] = True
    P["matches"] = int((m >= 0).sum())
    return P, m.astype(np.int32)


# ---- the case table --------------------------------------------------------------------------
# name -> (builder, paths the case must reach, least number of matches the oracle finds).  The
# match counts are conditions on the inputs, read once from the CPU oracle's run.

def _seg_rows(per_seg, nseg=16, per=256, start=0, step=1):
    return [s * per + start + step * j for s in range(nseg) for j in range(per_seg)]


def _mixed(masked=False):
    cl = [dict(cam=i % 2, q=[10 + i], t=[700 - i], tflip=(0, 20)) for i in range(40)]
    cl += [dict(cam=i % 2, q=list(range(100 + 5 * i, 103 + 5 * i)),
                t=list(range(300 + 6 * i, 304 + 6 * i)), tflip=(0, 12)) for i in range(20)]
    return build(300, 800, 2, cl, masked=masked, thresh=0.3)


def _listed_elsewhere():
    # query 0 passes with row 4 (distance 2), which query 1 lists but fails; query 1 passes with
    # row 9 (distance 10) only: its best depends on query 0 having taken row 4
    cl = [dict(cam=0, q=[0, 1], t=[4, 9], tflips=[2, 10], pass_for={4: 0, 9: 1})]
    return build(4, 12, 1, cl, thresh=0.004)


def _all_private():
    cl = [dict(cam=i % 2, q=[3 * i], t=[250 - 2 * i], tflip=(0, 20)) for i in range(30)]
    return build(120, 260, 2, cl, thresh=0.3, seed=3)


def _multi(thresh):
    t = _seg_rows(13, step=7)[:200]
    return build(80, 4096, 1, [dict(cam=0, q=list(range(70)), t=t, tflip=(10, 21))], thresh=thresh)


def _multi_all_taken():
    return build(72, 300, 1, [dict(cam=0, q=list(range(70)), t=list(range(3, 69)), tflip=(10, 21))])


def _early_break():
    # best 2 -> threshold 4; the three near keys fail the check, every other key of round 0 is
    # farther than 4, and 40 keys are left for a second round that must not be read
    t = list(range(5, 57)) + list(range(260, 312))
    tf = [2, 3, 4] + [30 + (i % 9) for i in range(101)]
    return build(8, 600, 1, [dict(cam=0, q=[1, 2], t=t, tflips=tf, passes=t[3:])], thresh=0.004)


def _last_key_at_threshold():
    # best 5 -> threshold 10; round 0 holds no passing key and ends on a key at exactly 10, the
    # winners (distance 10) are the first keys of round 1
    t = list(range(5, 85))
    tf = [5] + [8] * 62 + [10, 10, 10] + [30] * 14
    return build(8, 300, 1, [dict(cam=0, q=[1, 2], t=t, tflips=tf, passes=[t[64], t[65]])], thresh=0.004)


def _cap_over_only():
    cl = [dict(cam=0, q=[3, 4], t=_seg_rows(70), tflip=(0, 25)),
          dict(cam=0, q=[9], t=[4000], tflip=(0, 5))]
    return build(20, 4096, 1, cl, thresh=0.3)


def _cap_over_tail_winners():
    # three queries of 1504 keys each (94 per segment): over kTriWin without any slot over, and the
    # only passing rows are their three farthest keys
    t = _seg_rows(94)
    tf = [10 + (i % 10) for i in range(len(t))]
    for i in (-1, -2, -3):
        tf[i] = 20
    return build(6, 4096, 1, [dict(cam=0, q=[0, 2, 5], t=t, tflips=tf, passes=t[-3:])], thresh=0.004)


def _total(c):
    t = _seg_rows(64) + ([4090] if c == 1025 else [])
    return build(6, 4096, 1, [dict(cam=0, q=[1, 4], t=sorted(t), tflip=(5, 11))])


def _segment(c):
    t = list(range(300, 300 + c))
    return build(6, 1000, 1, [dict(cam=0, q=[1, 4], t=t, tflip=(5, 11)),
                              dict(cam=0, q=[2], t=[900], tflip=(0, 5))])


def _window_jump():
    heavy = _seg_rows(60, start=100)
    cl = [dict(cam=0, q=[0, 1], t=[5, 6, 7], tflip=(0, 10)),
          dict(cam=0, q=[2, 8], t=[20, 21], tflip=(0, 6)),       # one before, one after the block
          dict(cam=1, q=[3, 4, 5], t=heavy, tflip=(0, 25)),
          dict(cam=0, q=[9, 10], t=[8, 9, 10], tflip=(0, 10))]
    return build(16, 4096, 2, cl)


def _tiles(n2):
    per = -(-(-(-n2 // 16)) // 256) * 256
    rows = sorted({r for r in (0, 255, 256, 257, per - 1, per, per + 255, per + 256, n2 - 2, n2 - 1)
                   if 0 <= r < n2})
    return build(257, n2, 1, [dict(cam=0, q=[0, 255, 256], t=rows, tflip=(0, 20))])


def _one_by_one():
    return build(1, 1, 1, [dict(cam=0, q=[0], t=[0], tflip=(3, 4))])


def _one_camera():
    cl = [dict(cam=0, q=[4 * i, 4 * i + 1], t=[200 - 3 * i, 201 - 3 * i, 202 - 3 * i], tflip=(0, 15))
          for i in range(10)] + [dict(cam=0, q=[50 + i], t=[250 + i], tflip=(0, 15)) for i in range(10)]
    return build(70, 300, 1, cl, thresh=0.3)


def _eight_cameras():
    cl = [dict(cam=c, q=[10 * c, 10 * c + 3, 10 * c + 4], t=[90 * c + j for j in (1, 40, 41, 80)],
               tflip=(0, 15)) for c in range(8)]
    return build(96, 800, 8, cl)


def _eight_cameras_largest():
    n2 = (1 << 19) - 1
    per = 32768
    cl = [dict(cam=7, q=[0, 63], t=[0, n2 - 2, n2 - 1], tflip=(0, 10)),
          dict(cam=3, q=[5, 6, 7], t=[per - 1, per, per + 255, per + 256, 15 * per, 15 * per - 1], tflip=(0, 10)),
          dict(cam=0, q=[31], t=[(1 << 18) + 12345], tflip=(0, 10))]
    return build(64, n2, 8, cl)


def _entries(ns):
    k = {0: 0, 64: 32, 65: 31}[ns]
    cl = [dict(cam=i % 2, q=[3 * i, 3 * i + 1], t=[400 - 3 * i, 401 - 3 * i], tflip=(0, 10)) for i in range(k)]
    if ns == 65:
        cl.append(dict(cam=0, q=[100, 101, 102], t=[10, 11, 12], tflip=(0, 10)))
    cl += [dict(cam=i % 2, q=[110 + i], t=[20 + i], tflip=(0, 10)) for i in range(5)]
    return build(120, 420, 2, cl)


def _shared(nbytes, masked, seed=0):
    from tests import test_matcher as tm
    pr = tm._tri_problem_shared(seed, nbytes=nbytes)
    m1 = tm._masks(len(pr[0]), nbytes, seed + 10, keep=0.9) if masked else None
    m2 = tm._masks(len(pr[1]), nbytes, seed + 11, keep=0.9) if masked else None
    return from_arrays(*pr, 0.3, m1, m2)


def _duplicates():
    return build(8, 40, 1, [dict(cam=0, q=[0, 1, 2], t=[10, 5, 7, 20], tflips=[0, 0, 0, 0]),
                            dict(cam=0, q=[6], t=[30, 25], tflips=[0, 0])])


def _best_zero():
    cl = [dict(cam=0, q=[0, 1, 2], t=[5, 7, 9, 11, 12], tflips=[0, 0, 1, 2, 3], passes=[9, 11, 12]),
          dict(cam=0, q=[6], t=[30, 25], tflips=[0, 1], passes=[25]),
          dict(cam=0, q=[7], t=[31, 33], tflips=[1, 0], passes=[33])]
    return build(8, 40, 1, cl, thresh=0.004)


CASES = {
    "mixed": (_mixed, ("private_and_ordered_in_one_call", "q_private_won", "q_private_nomatch", "q_flagged",
                       "seq_pair", "seq_pair_second_sees_first_winner", "q_empty", "ens_first", "ens_same",
                       "radius_one_tile"), 60),
    "listed_elsewhere": (_listed_elsewhere, ("seq_nearest_already_taken", "seq_pair"), 2),
    "mixed_masked": (lambda: _mixed(True), ("private_and_ordered_in_one_call", "q_private_won", "q_flagged",
                                            "seq_pair"), 60),
    "all_private": (_all_private, ("ns_0", "q_private_won", "q_private_nomatch"), 10),
    "multi_all_pass": (lambda: _multi(1e9), ("seq_multi_round", "seq_multi_best_in_later_round", "ens_next",
                                             "seq_single_straddles_window"), 70),
    "multi_rare_pass": (lambda: _multi(0.004), ("seq_multi_round", "seq_multi_winner_after_best_round"), 1),
    "multi_all_taken": (_multi_all_taken, ("seq_multi_all_taken", "seq_multi_best_in_later_round"), 66),
    "early_break": (_early_break, ("seq_multi_early_break",), 0),
    "last_key_at_threshold": (_last_key_at_threshold, ("seq_multi_last_key_at_threshold",
                                                       "seq_multi_winner_after_best_round"), 2),
    "cap_over_only": (_cap_over_only, ("q_cap_over_only", "seq_rescan", "q_private_won"), 3),
    "cap_over_tail_winners": (_cap_over_tail_winners, ("q_cap_over_only", "seq_rescan_won"), 3),
    "total_1024": (lambda: _total(1024), ("seq_multi_round", "ens_next"), 2),
    "total_1025": (lambda: _total(1025), ("q_cap_over_only", "seq_rescan_won"), 2),
    "segment_96": (lambda: _segment(96), ("seq_multi_round", "q_private_won"), 3),
    "segment_97": (lambda: _segment(97), ("q_slot_over", "slot_overflow_pairs", "global_overflow", "seq_rescan_won",
                                          "seq_one_round"), 3),
    "window_jump": (_window_jump, ("ens_jump", "seq_pair_refused_span", "seq_pair", "seq_multi_round",
                                   "seq_one_round"), 9),
    "tiles_4097": (lambda: _tiles(4097), ("radius_multi_tile", "radius_partial_tile", "radius_empty_segments",
                                          "seq_one_round"), 3),
    "tiles_8193": (lambda: _tiles(8193), ("radius_multi_tile", "radius_partial_tile"), 3),
    "tiles_15": (lambda: _tiles(15), ("radius_empty_segments", "radius_partial_tile"), 3),
    "one_by_one": (_one_by_one, ("q_private_won", "ncams_1"), 1),
    "one_camera": (_one_camera, ("ncams_1", "private_and_ordered_in_one_call"), 10),
    "eight_cameras": (_eight_cameras, ("lds_over_64k", "q_flagged"), 8),
    "eight_cameras_largest": (_eight_cameras_largest, ("lds_over_64k", "radius_multi_tile", "q_flagged",
                                                       "q_private_won"), 6),
    "entries_0": (lambda: _entries(0), ("ns_0",), 5),
    "entries_64": (lambda: _entries(64), ("ns_64",), 69),
    "entries_65": (lambda: _entries(65), ("ns_65", "entry_chunks_multi"), 70),
    "duplicates": (_duplicates, ("seq_one_round", "q_private_won"), 4),
    "best_zero": (_best_zero, ("q_flagged", "q_private_nomatch", "q_private_won"), 1),
}
for _nb in (16, 32, 64):
    for _mk in (False, True):
        CASES["shared_%d%s" % (_nb, "_masked" if _mk else "")] = (
            functools.partial(_shared, _nb, _mk), ("seq_rescan", "slot_overflow_pairs", "global_overflow"), 50)


@functools.lru_cache(maxsize=None)
def get(name):
    """The case `name`, built once and shared (treat as read-only)."""
    return CASES[name][0]()


@functools.lru_cache(maxsize=None)
def reached(name):
    return paths(get(name))
