"""Scripted scenarios for the keyframe database, shared by the CPU and GPU tests and by the
fixture generator (tests/golden/gen_kfdb_ref.py).  A scenario is a vocabulary size and a list of
operations; `run` plays it on any database that has the interface of tests/np_kfdb.Database and
records what every query returns and the six members after it.

Operations (tuples):
  ("add", word, value, reloc_score_init)
  ("erase", slot)
  ("min", q_word, q_value, slots)                       -> keeps the result as the next loop's minScore
  ("loop", q_word, q_value, query_id, connected, min_score | None, neigh)   None = the last "min"
  ("reloc", q_word, q_value, query_id, neigh)
"""
import numpy as np

NEIGH = 10
NO_NEIGH = lambda n: np.full((n, NEIGH), -1, np.int32)   # noqa: E731


def _norm(v):
    v = np.asarray(v, np.float64)
    return v / v.sum() if len(v) else v


def rand_bow(rng, pool, length):
    """A BowVector of `length` distinct words of `pool`, L1-normalised values."""
    w = np.sort(rng.choice(pool, size=length, replace=False)).astype(np.uint32)
    return w, _norm(rng.uniform(0.2, 1.0, size=length))


def rand_neigh(rng, n, fill=0.7):
    ng = np.full((n, NEIGH), -1, np.int32)
    for s in range(n):
        k = int(rng.integers(0, NEIGH + 1)) if rng.random() < fill else 0
        ng[s, :k] = rng.integers(-1, n + 1, size=k)   # -1 = padding, n = not in the database
    return ng


def case_lengths():
    """BowVector lengths 0, 1, 63, 64, 65, 129; shared words at positions 0, 63, 64 and last; a
    keyframe sharing no word; a query of one word."""
    rng = np.random.default_rng(11)
    odd = np.arange(1, 729, 2)
    ops, shared = [], []
    for length in (0, 1, 63, 64, 65, 129, 40):
        w = np.sort(rng.choice(odd, size=length, replace=False)).astype(np.uint32)
        if length == 40:
            pass                                  # odd words only: shares nothing with the query
        else:
            for p in sorted({p for p in (0, 63, 64, length - 1) if 0 <= p < length}):
                w[p] -= 1                         # even, still above the odd word before it
                shared.append(int(w[p]))
        ops.append(("add", w, _norm(rng.uniform(0.2, 1.0, size=length)), 0.0))
    n = 7
    qw = np.unique(np.array(shared + [600, 602, 604], np.uint32))
    qv = _norm(rng.uniform(0.2, 1.0, size=len(qw)))
    ng = rand_neigh(rng, n)
    conn = np.zeros(n, np.uint8)
    ops.append(("min", qw, qv, [1, 3]))
    ops.append(("loop", qw, qv, 3, conn, 0.0, ng))
    ops.append(("reloc", qw, qv, 4, ng))
    one = np.array([shared[-1]], np.uint32)       # the last word of the 129-entry keyframe
    ops.append(("reloc", one, np.array([1.0]), 5, ng))
    ops.append(("loop", one, np.array([1.0]), 6, conn, 0.0, ng))
    empty = np.zeros(0, np.uint32)
    ops.append(("reloc", empty, np.zeros(0), 7, ng))
    return {"name": "lengths", "n_words": 729, "ops": ops}


def case_random(n, seed, n_words=729):
    """N keyframes over a small word pool: heavy sharing, erased keyframes in the middle, connected
    keyframes, a repeated query id, query id 0 against fresh members."""
    rng = np.random.default_rng(seed)
    pool = np.arange(0, min(n_words, 300))
    ops = []
    for s in range(n):
        w, v = rand_bow(rng, pool, int(rng.integers(1, 90)))
        ops.append(("add", w, v, 0.0))
    ng = rand_neigh(rng, n)
    q1 = rand_bow(rng, pool, 70)
    q2 = rand_bow(rng, pool, 50)
    conn = (rng.random(n) < 0.2).astype(np.uint8)
    none = np.zeros(n, np.uint8)
    ops.append(("loop", q1[0], q1[1], 0, none, 0.0, ng))        # id 0 == the fresh loop_query
    ops.append(("min", q1[0], q1[1], np.flatnonzero(conn).tolist()))
    ops.append(("loop", q1[0], q1[1], 5, conn, None, ng))
    ops.append(("loop", q1[0], q1[1], 5, conn, 0.0, ng))        # repeated id: nothing is listed
    ops.append(("reloc", q2[0], q2[1], 7, ng))
    if n > 2:
        ops.append(("erase", n // 2))
        ops.append(("erase", n // 3))
    ops.append(("reloc", q1[0], q1[1], 8, ng))                  # neighbours carry scores of id 7
    ops.append(("loop", q2[0], q2[1], 9, conn, 0.01, ng))
    ops.append(("reloc", q2[0], q2[1], 8, ng))                  # repeated reloc id
    return {"name": "random%d" % n, "n_words": n_words, "ops": ops}


def _single(v, w=10, extra=()):
    """A keyframe holding word w with value v (plus words that the query does not have)."""
    words = np.array(sorted([w] + list(extra)), np.uint32)
    vals = np.array([v if x == w else 0.25 for x in words.tolist()], np.float64)
    return words, vals


def case_retain_exact():
    """accScore == 0.75 * bestAccScore exactly: not retained (strict >).  A query of the single word
    10 with value 1.0 scores a keyframe holding (10, v), v <= 1, at exactly v."""
    ops = []
    for v, extra in ((0.375, ()), (0.5, (20,)), (0.40625, (30, 31))):
        w, val = _single(v, extra=extra)
        ops.append(("add", w, val, 0.0))
    q = (np.array([10], np.uint32), np.array([1.0]))
    ng = NO_NEIGH(3)
    ops.append(("reloc", q[0], q[1], 1, ng))
    ops.append(("loop", q[0], q[1], 1, np.zeros(3, np.uint8), 0.125, ng))
    return {"name": "retain_exact", "n_words": 729, "ops": ops}


def case_min_score_equal():
    """si == minScore exactly: kept (>=).  minScore comes from the min-score call over a slot list
    that names the keyframe itself."""
    ops = []
    for v in (0.5, 0.25, 0.625):
        w, val = _single(v)
        ops.append(("add", w, val, 0.0))
    q = (np.array([10], np.uint32), np.array([1.0]))
    ng = NO_NEIGH(3)
    ops.append(("min", q[0], q[1], [0, 2]))                    # 0.5
    ops.append(("loop", q[0], q[1], 2, np.zeros(3, np.uint8), None, ng))
    return {"name": "min_score_equal", "n_words": 729, "ops": ops}


def case_dedupe():
    """Two scored keyframes (slots 0 and 2) have the same best neighbour (slot 3); slot 1 stands for
    itself.  The output names slot 3 once, at its first list position."""
    ops = []
    for v in (0.3, 0.7, 0.35, 0.5):
        w, val = _single(v)
        ops.append(("add", w, val, 0.0))
    ng = NO_NEIGH(4)
    ng[0, 0] = 3
    ng[2, 1] = 3
    q = (np.array([10], np.uint32), np.array([1.0]))
    ops.append(("reloc", q[0], q[1], 1, ng))
    ops.append(("loop", q[0], q[1], 1, np.zeros(4, np.uint8), 0.0, ng))
    return {"name": "dedupe", "n_words": 729, "ops": ops}


def case_stale_reloc():
    """A neighbour with few shared words is not scored by the second query, so the accumulation reads
    the score the first query left; that value decides whether slot 1 is retained."""
    q2w = np.arange(100, 110, dtype=np.uint32)
    q2v = np.full(10, 0.1)
    ops = [("add", q2w.copy(), q2v.copy(), 0.0),                                  # A: all ten words
           ("add", q2w[:9].copy(), _norm(np.full(9, 1.0)), 0.0),                  # B: nine words
           ("add", np.array([109, 200, 201, 202], np.uint32), np.full(4, 0.25), 0.0)]   # N: one word
    ng = NO_NEIGH(3)
    ng[0, 0] = 2
    q1 = (np.array([200, 201, 202], np.uint32), _norm(np.full(3, 1.0)))
    ops.append(("reloc", q1[0], q1[1], 1, ng))          # scores N only
    ops.append(("reloc", q2w, q2v, 2, ng))
    return {"name": "stale_reloc", "n_words": 729, "ops": ops}


def case_connected():
    """Connected keyframes: not listed, loop_query unchanged, loop_words ends at 1."""
    rng = np.random.default_rng(5)
    pool = np.arange(0, 60)
    ops = []
    for s in range(6):
        w, v = rand_bow(rng, pool, 30)
        ops.append(("add", w, v, 0.0))
    q = rand_bow(rng, pool, 30)
    conn = np.array([0, 1, 0, 1, 0, 0], np.uint8)
    ng = rand_neigh(rng, 6, fill=1.0)
    ops.append(("min", q[0], q[1], [1, 3]))
    ops.append(("loop", q[0], q[1], 4, conn, 0.0, ng))
    return {"name": "connected", "n_words": 729, "ops": ops}


def all_cases():
    return [case_lengths(), case_random(1, 21), case_random(65, 22), case_random(301, 23), case_retain_exact(),
            case_min_score_equal(), case_dedupe(), case_stale_reloc(), case_connected()]


def run(db, case):
    """Play a scenario -> list of records (dicts of numpy arrays / floats), one per query."""
    recs, last_min = [], 1.0
    for op in case["ops"]:
        kind = op[0]
        if kind == "add":
            db.add(op[1], op[2], op[3])
        elif kind == "erase":
            db.erase(op[1])
        elif kind == "min":
            last_min = db.min_score(op[1], op[2], list(op[3]))
            recs.append({"kind": "min", "min_score": np.float64(last_min)})
        else:
            if kind == "loop":
                ms = last_min if op[5] is None else op[5]
                r = db.detect_loop(op[1], op[2], op[3], op[4], ms, op[6])
            else:
                r = db.detect_reloc(op[1], op[2], op[3], op[4])
            rec = {"kind": kind, "candidates": np.asarray(r["candidates"], np.int32),
                   "common": np.asarray(r["common"], np.int32), "score": np.asarray(r["score"], np.float64)}
            rec.update(db.members())
            recs.append(rec)
    return recs


def same(a, b):
    """Exact comparison of two record lists: integers equal, doubles equal as 64-bit patterns."""
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x["kind"] == y["kind"] and x.keys() == y.keys(), i
        for k in x:
            if k == "kind":
                continue
            u, v = np.asarray(x[k]), np.asarray(y[k])
            assert u.shape == v.shape, (i, k, u.shape, v.shape)
            if u.dtype == np.float64:
                u, v = u.view(np.uint64), np.asarray(v, np.float64).view(np.uint64)
            assert np.array_equal(u, v), (i, x["kind"], k, x[k], y[k])
