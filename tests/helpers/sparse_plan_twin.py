"""NumPy twin of K5's route choice (tsu_sparse_classify / SparseSystem.plan, csrc/sparse_host.h), written from the rules in the
classifier's comments, and the graphs on which tests/test_sparse_plan_cpu.py and tests/test_sparse_routes_gpu.py pin it.

Rules.  Everything is in POSITION space: position p holds site order[p]; row p is the CSR row of that site with its columns replaced
by the neighbours' positions (kept in ascending order of the neighbours' SITE numbers).
  * n <= 32768: the whole system runs on k5_small (route 2), whatever its classes look like; the record keeps what the rules below
    find for the class, with v4 = 0 (no stencil kernel is launched).
  * A class [pb, pe) of fewer than 4 * 64 + 2 rows is generic (route 0).  Otherwise its MIDDLE row pm = pb + (pe - pb) // 2 sets the
    pattern: deg = its length (1 .. 4, else generic), Jv = its first coupling, the bias of pm, the offsets col - pm, and
    site_stride = order[pm + 1] - order[pm].
  * A row p FITS if it has deg entries, the pattern's bias, order[p] = order[pm] + site_stride (p - pm), and every entry has the
    coupling Jv and the pattern's offset, which is not 0 (no self-loop).
  * lo / hi = the number of leading / trailing rows that do not fit; each at most 64, and every row in between must fit.  Else generic.
  * Pairs (TSU_K5_PAIR != 0): classes c < c2, both regular and unpaired with site_stride 2, sites ascending by 2 over the WHOLE class,
    order[pb_c] ^ 1 == order[pb_c2], and the regular rows of c2 end no later (by index) than class c does: c gets pair 1, c2 pair 2.
    The first such c2 wins.
  * v4 (TSU_K5_V4 != 0): pb % 4 == 0, and for pair 1 also the partner's pb % 4 == 0.
A record: route, deg, lo, hi, site_stride, pair, other, v4, o_lo, o_n (o_lo, o_n: pair 1 only -- the partner's lo and the number of
its regular rows).  A class that is not regular: everything else 0, other -1.
"""
import numpy as np
import scipy.sparse as sp

FIELDS = ("route", "deg", "lo", "hi", "site_stride", "pair", "other", "v4", "o_lo", "o_n")
MAX_DEG, EDGE, SMALL_MAX = 4, 64, 32768


def _record(**kw):
    rec = dict.fromkeys(FIELDS, 0)
    rec["other"] = -1
    rec.update(kw)
    return rec


def classify(row_ptr, col_idx, values, bias, color_offsets, order, use_stencil=True, use_pairs=True, use_v4=True):
    rp = np.asarray(row_ptr, dtype=np.int64)
    ci = np.asarray(col_idx, dtype=np.int64)
    va = np.asarray(values, dtype=np.float64)
    off = np.asarray(color_offsets, dtype=np.int64)
    order = np.asarray(order, dtype=np.int64)
    n = rp.size - 1
    n_colors = off.size - 1
    small = n <= SMALL_MAX
    b = np.zeros(n) if bias is None else np.asarray(bias, dtype=np.float64)
    pos_of = np.empty(n, dtype=np.int64)
    pos_of[order] = np.arange(n)
    length = np.diff(rp)[order]            # row length, bias and first entry of every POSITION
    bias_p = b[order]
    start = rp[:-1][order]
    classes = []
    for c in range(n_colors):
        pb, pe = int(off[c]), int(off[c + 1])
        classes.append(None)
        if not use_stencil or pe - pb < 4 * EDGE + 2:
            continue
        pm = pb + (pe - pb) // 2
        deg = int(length[pm])
        if deg < 1 or deg > MAX_DEG:
            continue
        Jv = va[start[pm]]
        offs = pos_of[ci[start[pm]:start[pm] + deg]] - pm
        stride = int(order[pm + 1] - order[pm])
        p = np.arange(pb, pe)
        fits = (length[p] == deg) & (bias_p[p] == bias_p[pm]) & (order[p] == order[pm] + stride * (p - pm))
        q = p[fits]                        # rows of the right length: compare their entries with the pattern's
        ok = np.ones(q.size, dtype=bool)
        for i in range(deg):
            e = start[q] + i
            ok &= (va[e] == Jv) & (pos_of[ci[e]] - q == offs[i]) & (pos_of[ci[e]] != q)
        fits[fits] = ok
        good = np.flatnonzero(fits)
        if good.size == 0:
            continue
        lo, hi = int(good[0]), int(p.size - 1 - good[-1])
        if lo > EDGE or hi > EDGE or not fits[lo:p.size - hi].all():
            continue
        classes[c] = dict(deg=deg, lo=lo, hi=hi, stride=stride, pb=pb, pe=pe, pair=0, other=-1)
    for c in range(n_colors):
        A = classes[c]
        if not use_pairs or A is None or A["pair"] or A["stride"] != 2:
            continue
        for c2 in range(c + 1, n_colors):
            B = classes[c2]
            if B is None or B["pair"] or B["stride"] != 2 or (order[A["pb"]] ^ 1) != order[B["pb"]]:
                continue
            whole = all(np.array_equal(order[X["pb"]:X["pe"]], order[X["pb"]] + 2 * np.arange(X["pe"] - X["pb"])) for X in (A, B))
            if not whole or (B["pe"] - B["hi"]) - B["pb"] > A["pe"] - A["pb"]:
                continue
            A.update(pair=1, other=c2)
            B.update(pair=2, other=c)
            break
    out = []
    for S in classes:
        if S is None:
            out.append(_record(route=2 if small else 0))
            continue
        o = classes[S["other"]] if S["pair"] == 1 else None
        v4 = not small and use_v4 and S["pb"] % 4 == 0 and (o is None or o["pb"] % 4 == 0)
        out.append(_record(route=2 if small else 1, deg=S["deg"], lo=S["lo"], hi=S["hi"], site_stride=S["stride"], pair=S["pair"], other=S["other"],
                           v4=int(v4), o_lo=o["lo"] if o else 0, o_n=(o["pe"] - o["hi"]) - (o["pb"] + o["lo"]) if o else 0))
    return out


# ------------------------------------------------------------------ the graphs of the route tests

def banded(n, even, odd, v_even, v_odd):
    """Row i couples to i + d for d in `even` (even i, coupling v_even) or `odd` (odd i, v_odd), where that is a site: CSR, columns
    ascending, no explicit zeros.  (Rows need not be symmetric: the sweep reads row i only.)"""
    rows, cols, vals = [], [], []
    for par, ds, v in ((0, even, v_even), (1, odd, v_odd)):
        i = np.arange(par, n, 2)
        for d in ds:
            j = i + d
            k = (j >= 0) & (j < n)
            rows.append(i[k])
            cols.append(j[k])
            vals.append(np.full(int(k.sum()), v))
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    A.sort_indices()
    return A


def _even_odd(n, odd_first=False, descending=False):
    ev, od = np.arange(0, n, 2), np.arange(1, n, 2)
    if descending:
        ev, od = ev[::-1], od[::-1]
    first, second = (od, ev) if odd_first else (ev, od)
    return np.array([0, first.size, n], np.int32), np.concatenate([first, second]).astype(np.int32)


def _class_bias(n, offsets, order, values):
    bias = np.empty(n)
    for c, v in enumerate(values):
        bias[order[offsets[c]:offsets[c + 1]]] = v
    return bias


B0, B1, B2, B_OTHER = 0.3, -0.7, 0.1, 1.1   # class-dependent bias: thr != thr_other in every pair


def graph(name, n):
    """(A, bias, offsets, order, classes, pairs): the CSR matrix, a class-dependent bias, the colouring (the one tsu.graph.color_graph
    gives unless the case says otherwise) and, per class, the literal (deg, lo, hi, site_stride) expected of the classifier -- None: a
    generic class -- and whether classes 0 and 1 form a pair (with TSU_K5_PAIR on)."""
    other = {}
    if name == "dimers":
        A, cls, pairs = banded(n, [1], [-1], 0.8, 0.8), [(1, 0, 0, 2), (1, 0, 0, 2)], True
    elif name == "degree3":
        A, cls, pairs = banded(n, [-1, 1, 3], [-3, -1, 1], -0.6, -0.6), [(3, 1, 1, 2), (3, 1, 1, 2)], True
    elif name == "degree4":
        A, cls, pairs = banded(n, [-3, -1, 1, 3], [-3, -1, 1, 3], 0.8, 0.8), [(4, 2, 1, 2), (4, 1, 2, 2)], True
    elif name == "asymmetric":
        A, cls, pairs = banded(n, [-3, -1, 1, 3], [-1, 1], 0.8, -0.5), [(4, 2, 1, 2), (2, 0, 1, 2)], True
    elif name == "halves":  # the chain relabelled: its even positions are sites 0 .. n/2 - 1, its odd ones sites n/2 .. n - 1
        h = n // 2
        i = np.arange(h)
        rows = np.concatenate([i[1:], i])
        cols = np.concatenate([h + i[1:] - 1, h + i])
        M = sp.coo_matrix((np.full(rows.size, 0.8), (rows, cols)), shape=(n, n))
        A = (M + M.T).tocsr()
        A.sort_indices()
        cls, pairs = [(2, 1, 0, 1), (2, 0, 1, 1)], False
        offsets, order = np.array([0, h, n], np.int32), np.arange(n, dtype=np.int32)
    elif name == "strip":  # triangular strip, three classes by site mod 3 (n a multiple of 3)
        i = np.arange(n)
        rows = np.concatenate([i[:-1], i[:-2]])
        cols = np.concatenate([i[:-1] + 1, i[:-2] + 2])
        M = sp.coo_matrix((np.full(rows.size, 0.5), (rows, cols)), shape=(n, n))
        A = (M + M.T).tocsr()
        A.sort_indices()
        cls, pairs = [(4, 1, 0, 3), (4, 1, 1, 3), (4, 0, 1, 3)], False
        offsets = np.array([0, n // 3, 2 * (n // 3), n], np.int32)
        order = np.concatenate([np.arange(c, n, 3) for c in range(3)]).astype(np.int32)
    elif name.startswith("chain"):
        A = banded(n, [-1, 1], [-1, 1], 0.8, 0.8)
        cls, pairs = [(2, 1, 0, 2), (2, 0, 1, 2)], True
        if name.startswith("chain_first"):      # the first k even sites with another bias
            k = int(name[len("chain_first"):])
            other = {2 * j: B_OTHER for j in range(k)}
            cls[0] = (2, k, 0, 2) if k <= 64 else None
        elif name == "chain_both_ends":         # the first 3 even sites and the last 61 odd sites
            other = {2 * j: B_OTHER for j in range(3)}
            other.update({n - 1 - 2 * j: B_OTHER for j in range(61)})
            cls = [(2, 3, 0, 2), (2, 0, 61, 2)]
        elif name == "chain_interior":          # one even site a quarter of the way along
            other = {2 * (n // 8): B_OTHER}
            cls[0] = None
        elif name == "chain_odd_first":         # n odd: the odd sites, then the even ones -- the second class is one longer
            cls = [(2, 0, 0, 2), (2, 1, 1, 2)]
            offsets, order = _even_odd(n, odd_first=True)
        elif name == "chain_descending":        # both classes in descending site order (fixed offsets need the same direction in both)
            cls, pairs = [(2, 0, 1, -2), (2, 1, 0, -2)], False
            offsets, order = _even_odd(n, descending=True)
        else:
            assert name == "chain", name
        pairs = pairs and None not in cls
    else:
        raise ValueError(name)
    if name not in ("halves", "strip", "chain_odd_first", "chain_descending"):
        offsets, order = _even_odd(n)
    bias = _class_bias(n, offsets, order, (B0, B1, B2)[:len(cls)])
    for site, v in other.items():
        bias[site] = v
    return A, bias, offsets, order, cls, pairs


def expected_plan(offsets, classes, pairs, use_pairs=True, use_v4=True):
    """The full records from the literals of `graph`: pair / other from `pairs`, v4 from pb % 4 (and the partner's), o_lo / o_n from the
    partner's literals."""
    out = []
    small = int(offsets[-1]) <= SMALL_MAX   # route 2: the classes as classified, nothing launched four positions per thread
    for c, lit in enumerate(classes):
        if lit is None:
            out.append(_record(route=2 if small else 0))
            continue
        deg, lo, hi, stride = lit
        rec = _record(route=2 if small else 1, deg=deg, lo=lo, hi=hi, site_stride=stride)
        v4 = not small and use_v4 and offsets[c] % 4 == 0
        if pairs and use_pairs and c < 2:
            rec.update(pair=c + 1, other=1 - c)
            if c == 0:
                _, o_lo, o_hi, _ = classes[1]
                rec.update(o_lo=o_lo, o_n=int(offsets[2] - offsets[1]) - o_lo - o_hi)
                v4 = v4 and offsets[1] % 4 == 0
        rec["v4"] = int(v4)
        out.append(rec)
    return out


def thresholds(deg, Jv, bias, T, sigmoid):
    """thr[k], k = 0 .. deg, as k5_thresholds computes them: the field of k set neighbours summed edge by edge, then the bias;
    ceil(p 2^53), and 2^53 for p = 1.  `sigmoid`: the oracle's (clamped at +-20)."""
    import math
    out = []
    for k in range(deg + 1):
        F = 0.0
        for _ in range(k):
            F += Jv * 1.0
        F += bias
        p = sigmoid(F / T)
        out.append(1 << 53 if p >= 1.0 else int(math.ceil(math.ldexp(p, 53))))
    return out
