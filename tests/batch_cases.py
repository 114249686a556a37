"""TEST UTILITY: the edge LPs, the feature detector, the K-member host stand-in and the scenario of tests/test_batch_attempts_gpu.py (the
shared-matrix lockstep batch, cuopt_amd/csrc/kernels_batch.hip and batch_common.hpp, checked stage by stage with
tests/attempt_reference.py).  tests/test_batch_cases.py runs all of it on the host.  numpy only.

THE EDGE LP (edge_lp).  Both matrices -- A by rows and A^T by rows -- are built from explicit ROW-LENGTH LISTS, so that the blocks of 512
rows the batched products walk (batch_block_sums) meet the shapes features() lists.  The products cut the rows into workgroups along the
single layouts' boundaries, which two greedy rules decide from the row offsets alone (restated here as stream_cuts and panel_cuts: the
GPU test takes the boundaries from the batch itself and asserts the features on THOSE):
    CSR stream   a block takes rows while its entries stay within 2044 (kNnzBlock), at most 1024 rows (kMaxRowsPerBlock)
    panels       with CUOPT_AMD_TUNE panel_nnz=2048: rows while the entries stay within 2048, at most 3584 rows (kPanelMaxRows)
No row has more than 128 entries, so a block of ONE row exists only where a row cap ends the block in front of the matrix's last row.
A side's rows are, in this order:
    head     blocks of 2040 entries each whose first row has 128 entries -- 2040 + 128 is beyond either limit, so both rules cut in
             front of every one of them: 512 rows (the chunk-boundary rows PRE in front), 513 rows, 662 rows (1025 entries in the
             first 512 rows), 16 rows (the A^T side: two of these);
    uniform  the OTHER side's columns: u rows of exactly 34 entries = whole blocks of 60 rows, 2040 entries, under both rules;
    tail     ten stretches of 512 rows holding 1024, 0, 1024, 513, 512, 257, 256, 494, 0, 0 entries, then ONE empty row.  CSR stream:
             five blocks of 1024 rows by the row cap.  Panels: 1024 + 0 + 1024 = 2048 fill one panel of 1536 rows, the next takes 3584
             rows by the row cap and ends where the fifth stream block ends.  Under both rules the last row is a block of its own: nr = 1,
             no entries, off[r0] == nnz -- and both walk the ten stretches as blocks of 512 rows.
The tail is 1536 + 3584 + 1 rows so that nr = 1 holds for both layouts of ONE LP: here the capped panel starts behind a full first
panel and ends after 5 * 1024 rows, on a stream block's boundary.  With the head (1703 / 1719 rows) and the uniform part (420 / 360
rows) that gives 7244 x 7200; 24 480 + 2 040 nonzeros.  (A tail of 3585 rows also works -- 2040 entries in its rows 2048 .. 2559 and 8
in row 2560 shift the stream blocks by 512 -- but its one panel then has no entry to spare, and the six small counts would each need
a head block of more than 512 rows: more than 8 000 rows.  Nothing smaller than this LP was found; that none exists is not claimed.)
The pattern: a side's designed rows take consecutive entries of a stream that deals the other side's u uniform columns round and round,
column (p mod u) * 11 mod u for entry p.  11 has the inverse 131 modulo 360 and 191 modulo 420, so two entries of a row (at most 127
apart in the stream) never sit in adjacent columns, and two adjacent rows never share a column: no run of consecutive columns anywhere.

features() only REPORTS which edges a side carries under given boundaries; the tests assert that every name of FEATURES is reported.

THE SCENARIO (run_batch_scenario) and what is asserted per attempt and member (batch_attempt) are described in
tests/test_batch_attempts_gpu.py; Member / BatchStandIn put K float64 restatements behind the batch's two hooks so that
tests/test_batch_cases.py can run the same scenario, and three wrong variants of them, without a device."""
import collections

import numpy as np

import attempt_reference as ar
import attempt_scenario as sc

INF = np.inf
KBT, MAX_ROW = 512, 128
STREAM_NNZ, STREAM_ROWS = 2044, 1024
PANEL_NNZ, PANEL_ROWS = 2048, 3584
TUNE = dict(panel_seg=0, dense=0, panel_nnz=PANEL_NNZ, slab_bytes=4096)
BLOCK, UNIFORM, STRIDE = 2040, 34, 11
PRE = [128, 128, 0, 128, 64, 128, 64, 128, 0, 128, 128, 0, 128]  # ends at 128 256 256 384 448 576 640 768 768 896 1024 1024 1152
TAIL = [1024, 0, 1024, 513, 512, 257, 256, 494, 0, 0]
FEATURES = ("nch=0 in the middle", "empty last block", "nch=1", "nch=2", "nch=3", "CHUNK entries", "CHUNK+1 entries", "2*CHUNK entries",
            "128-entry row across a boundary", "row starts on a boundary", "row ends on a boundary", "empty row on a boundary",
            "nr=1", "nr<64", "nr=512", "nr=513", "nr ragged", "empty row", "empty column")


def chunk(K):
    """BatchGeometry<K>::CHUNK"""
    return 256 if K > 8 else 512


# ---- the two cutting rules, restated ----------------------------------------------------------------------------------------------------
def _greedy(off, limit, cap):
    off, rows, cuts, start = np.asarray(off, np.int64), len(off) - 1, [0], 0
    while start < rows:
        last = min(rows, start + cap)
        end = int(np.searchsorted(off[start:last + 1], off[start] + limit, side="right")) - 1 + start
        end = max(end, start + 1)
        cuts.append(end)
        start = end
    return np.array(cuts, np.int64)


def stream_cuts(off):
    """build_row_blocks (cuopt_amd/csrc/kernels_stream.hip) for rows of at most 128 entries"""
    return _greedy(off, STREAM_NNZ, STREAM_ROWS)


def panel_cuts(off):
    """panel_plan's cut (cuopt_amd/csrc/kernels_panel.hip) at the target 2048, no row with a workgroup of its own"""
    return _greedy(off, PANEL_NNZ, PANEL_ROWS)


# ---- which edges a side carries -----------------------------------------------------------------------------------------------------------
def features(off, row0, K, idx=None, ncols=None):
    """off: a side's CSR offsets, row0: the W + 1 block boundaries of its product (SharedMatrixBatch.view), K: the batch's width
    -> the set of FEATURES present ("empty column" only with the side's column indices and column count)"""
    off, row0 = np.asarray(off, np.int64), np.asarray(row0, np.int64)
    CH, found, blocks = chunk(K), set(), []
    for w in range(len(row0) - 1):
        r0, nr = int(row0[w]), int(row0[w + 1] - row0[w])
        for name, hit in (("nr=1", nr == 1), ("nr<64", 1 < nr < 64), ("nr=512", nr == 512), ("nr=513", nr == 513), ("nr ragged", 513 < nr < 1024)):
            if hit:
                found.add(name)
        for b0 in range(0, nr, KBT):
            a, b = r0 + b0, r0 + min(b0 + KBT, nr)
            eb0, eb1 = int(off[a]), int(off[b])
            count = eb1 - eb0
            nch = -(-count // CH)
            blocks.append(count)
            if 1 <= nch <= 3:
                found.add("nch=%d" % nch)
            for name, hit in (("CHUNK entries", count == CH), ("CHUNK+1 entries", count == CH + 1), ("2*CHUNK entries", count == 2 * CH)):
                if hit:
                    found.add(name)
            k0, k1 = off[a:b], off[a + 1:b + 1]
            for c in range(1, nch):
                edge = eb0 + c * CH
                for name, hit in (("128-entry row across a boundary", ((k1 - k0 == MAX_ROW) & (k0 < edge) & (k1 > edge)).any()),
                                  ("row starts on a boundary", ((k1 > k0) & (k0 == edge)).any()), ("row ends on a boundary", ((k1 > k0) & (k1 == edge)).any()),
                                  ("empty row on a boundary", ((k1 == k0) & (k0 == edge)).any())):
                    if hit:
                        found.add(name)
    if any(c == 0 for c in blocks[:-1]):
        found.add("nch=0 in the middle")
    if blocks and blocks[-1] == 0:
        found.add("empty last block")
    if (np.diff(off) == 0).any():
        found.add("empty row")
    if idx is not None and (np.bincount(np.asarray(idx, np.int64), minlength=int(ncols)) == 0).any():
        found.add("empty column")
    return found


def jag_unroll(K, waves):
    """JagBatchGeometry<K, WAVES>::U: the diagonals a lane requests per round"""
    return max(1, min(8, (16 if waves == 16 else 32) // K))


JAG_FEATURES = ("pass of fewer than 64 rows", "kmax not a multiple of U", "row without nonzeros", "several blocks")


def jag_features(off, row0, K, waves):
    """the paths of batch_jag_sums a jagged side reaches under the block boundaries row0 (SharedMatrixBatch.view): build_jag sorts a
    block's rows of 1 .. 128 entries by length, longest first, and cuts them into passes of 64 (only a block's last pass is shorter;
    it is the last of its wave's share, so the wave walks it as a pass of its own); a pass's kmax is its first row's length; rows
    without nonzeros are in no pass and keep the zeroed strip entry"""
    off, row0, U, found = np.asarray(off, np.int64), np.asarray(row0, np.int64), jag_unroll(K, waves), set()
    lens = np.diff(off)
    if len(row0) > 2:
        found.add("several blocks")
    for a, b in zip(row0[:-1], row0[1:]):
        rows = np.sort(lens[a:min(b, len(lens))])[::-1]
        if (rows == 0).any():
            found.add("row without nonzeros")
        rows = rows[rows > 0]
        if len(rows) % 64:
            found.add("pass of fewer than 64 rows")
        if (rows[::64] % U != 0).any():
            found.add("kmax not a multiple of U")
    return found


# ---- the edge LP ------------------------------------------------------------------------------------------------------------------------------
def _fill(rng, rows, count, first=0):
    """`rows` row lengths of at most 128 summing to `count`, many of them 0; the first one is `first` where given"""
    out = np.zeros(rows, np.int64)
    out[0] = first
    left = count - first
    assert left >= 0 and (left == 0 or rows > 1)
    if left:
        q = min(rows - 1, max(-(-left // 100), min(left, rows // 3)))
        at = 1 + rng.choice(rows - 1, size=q, replace=False)
        out[at] = 1
        left -= q
        while left > 0:
            j = at[rng.integers(q)]
            add = min(left, MAX_ROW - out[j], int(rng.integers(1, 40)))
            out[j] += add
            left -= add
    return out.tolist()


def designed_rows(rng, small_blocks):
    """(head, tail) row lengths of one side"""
    head = PRE + _fill(rng, KBT - len(PRE), BLOCK - sum(PRE))                                       # 512 rows, the boundary rows in front
    head +=_fill(rng, KBT, BLOCK - MAX_ROW, MAX_ROW) + [MAX_ROW]                                   # 513 rows
    head += _fill(rng, KBT, 1025, MAX_ROW) + _fill(rng, 150, BLOCK - 1025)                          # 662 rows: 1025 | 1015 entries
    for _ in range(small_blocks):
        head += [MAX_ROW] * 15 + [BLOCK - 15 * MAX_ROW]                                             # 16 rows
    tail = []
    for t, count in enumerate(TAIL):
        tail += _fill(rng, KBT, count, MAX_ROW if t == 0 else 5 if t == 3 else 0) if count else [0] * KBT
    return head, tail + [0]


def _deal(lengths, u):
    """(row, column) of every entry: rows of the given lengths over u columns of exactly sum / u entries each"""
    total = int(np.sum(lengths))
    assert total % (UNIFORM * 60) == 0 and total == UNIFORM * u, (total, u)
    p = np.arange(total)
    return np.repeat(np.arange(len(lengths)), lengths), (p % u) * STRIDE % u


def edge_lp(seed=5):
    """-> (p, x0, y0): the LP as a dict (x_star: a point strictly inside every inequality), a start"""
    rng = np.random.default_rng(seed)
    (head_a, tail_a), (head_t, tail_t) = designed_rows(rng, 1), designed_rows(rng, 2)
    len_a, len_t = np.array(head_a + tail_a), np.array(head_t + tail_t)
    u_p, u_q = int(len_a.sum()) // UNIFORM, int(len_t.sum()) // UNIFORM   # the columns P's rows use, the rows Q's columns make
    m, n = len(len_a) + u_q, len(len_t) + u_p
    ra, ca = _deal(len_a, u_p)  # P: A's designed rows over the columns [len(head_t), len(head_t) + u_p)
    rt, ct = _deal(len_t, u_q)  # Q: A^T's designed rows over A's rows [len(head_a), len(head_a) + u_q)
    rows = np.concatenate([np.where(ra < len(head_a), ra, ra + u_q), len(head_a) + ct])
    cols = np.concatenate([len(head_t) + ca, np.where(rt < len(head_t), rt, rt + u_p)])
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    values = rng.uniform(0.5, 2.0, len(rows)) * rng.choice([-1.0, 1.0], len(rows))
    off = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))]).astype(np.int32)
    x = rng.uniform(0.5, 1.5, n)
    act = np.bincount(rows, weights=values * x[cols], minlength=m)
    lo, hi, kind = row_bounds(act, rng)
    # a dual-feasible objective: c = A^T y + z with y of the rows' signs and z >= 0, so that the LP is bounded
    yd = np.abs(rng.standard_normal(m)) * np.choose(kind, [-1.0, 1.0, rng.choice([-1.0, 1.0], m), 0.0, 0.0])
    c = np.bincount(cols, weights=values * yd[rows], minlength=n) + 0.5 * np.abs(rng.standard_normal(n))
    p = dict(m=m, n=n, offsets=off, indices=cols.astype(np.int32), values=values, c=c, lb=np.zeros(n), ub=np.full(n, INF), lo=lo, hi=hi, x_star=x,
             activity=act, heads=(len(head_a), len(head_t)), uniform=(u_q, u_p))
    return p, np.abs(rng.standard_normal(n)), rng.standard_normal(m)


def row_bounds(act, rng):
    """a fifth each: <= act + 0.3, >= act - 0.3, = act, free, act - 0.5 <= . <= act + 0.5 -> (lo, hi, kind)"""
    m = len(act)
    kind = rng.integers(0, 5, m)
    lo = np.choose(kind, [np.full(m, -INF), act - 0.3, act, np.full(m, -INF), act - 0.5])
    hi = np.choose(kind, [act + 0.3, np.full(m, INF), act, np.full(m, INF), act + 0.5])
    return lo, hi, kind


def nonuniform_bounds(p, seed):
    """variable bounds around x_star on a third of the columns each: neither lb nor ub is one value throughout"""
    rng = np.random.default_rng(seed)
    x, n = p["x_star"], p["n"]
    pick = rng.integers(0, 3, n)
    return np.where(pick == 0, np.maximum(0.0, x - 0.4 * rng.random(n)), 0.0), np.where(pick == 1, x + 0.4 * rng.random(n), INF)


def members(p, K, uniform_parent=True):
    """the K members' (lb, ub, lo, hi, how): how = "parent" | "clone" | "reset-back" (a clone with other bounds, then reset to these).
    Member 1 has non-uniform bounds, 2 is reset BACK to the uniform ones, 3 has row bounds of its own (other kinds per row: infinite
    sides, equality rows), the rest are further variants; uniform_parent=False: the parent has non-uniform bounds itself."""
    lb0, ub0 = (p["lb"], p["ub"]) if uniform_parent else nonuniform_bounds(p, 90)
    out = [(lb0, ub0, p["lo"], p["hi"], "parent")]
    for l in range(1, K):
        lb, ub = nonuniform_bounds(p, 100 + l)
        if l == 2:
            out.append((p["lb"], p["ub"], p["lo"], p["hi"], "reset-back"))
        elif l == 3:
            lo, hi, _ = row_bounds(p["activity"], np.random.default_rng(77))
            out.append((lb, ub, lo, hi, "clone"))
        else:
            out.append((lb, ub, p["lo"], p["hi"], "clone"))
    return out


def banded_edge_lp(seed=9, m=2311, n=2203, band=90):
    """the jagged case's LP: a band of scattered columns (every other column at most), rows of 0 .. 14 entries with stretches of empty
    rows, a few empty columns -> (p, x0, y0)"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 15, m)
    lens[rng.random(m) < 0.08] = 0
    lens[700:790] = 0
    lens[m - 37:] = 0
    rows, cols = [], []
    for i in range(m):
        centre = int(i * (n - 1) / (m - 1))
        window = np.arange(max(0, centre - band), min(n, centre + band), 2)
        window = window[(window % 97) != 13]  # (columns 13, 110, ... stay empty)
        pick = np.sort(rng.choice(window, size=int(lens[i]), replace=False))
        rows += [i] * len(pick)
        cols += pick.tolist()
    rows, cols = np.array(rows), np.array(cols)
    values = rng.uniform(0.5, 2.0, len(rows)) * rng.choice([-1.0, 1.0], len(rows))
    off = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))]).astype(np.int32)
    x = rng.uniform(0.5, 1.5, n)
    act = np.bincount(rows, weights=values * x[cols], minlength=m)
    lo, hi, kind = row_bounds(act, rng)
    yd = np.abs(rng.standard_normal(m)) * np.choose(kind, [-1.0, 1.0, rng.choice([-1.0, 1.0], m), 0.0, 0.0])
    c = np.bincount(cols, weights=values * yd[rows], minlength=n) + 0.5 * np.abs(rng.standard_normal(n))
    p = dict(m=m, n=n, offsets=off, indices=cols.astype(np.int32), values=values, c=c, lb=np.zeros(n), ub=np.full(n, INF), lo=lo, hi=hi, x_star=x,
             activity=act)
    return p, np.abs(rng.standard_normal(n)), rng.standard_normal(m)


def feasible(p, lb, ub, lo, hi):
    """x_star satisfies the member's bounds"""
    x, act = p["x_star"], p["activity"]
    return bool((lb <= x).all() and (x <= ub).all() and (lo <= act + 1e-9).all() and (act - 1e-9 <= hi).all())


# ---- the scenario ---------------------------------------------------------------------------------------------------------------------------------
def left_to_right(S, prob, ctl, st):
    """the trial iterate of the panel and stream sides, every row and column summed left to right from once-rounded products (the
    order kernels_batch.hip promises): dict(xn, xbar, y, aty)"""
    p = ar.primal(prob, ctl, st)
    y = ar.dual_f64(prob, ctl, st, ar.rowsums_f64(prob["A_VALUES"], p["xbar"], S.off, S.idx))
    return dict(p, y=y, aty=ar.rowsums_f64(prob["AT_VALUES"], y, S.t_off, S.t_rows))


def _untouched(tag, before, after, parts_before, parts_after):
    for k in ar.STATE:
        assert ar.bits_equal(after[k], before[k]), (tag, "a resting member's buffer moved", k, ar._first(after[k], before[k]))
    cb, ca = before["ctl"], after["ctl"]
    for k in ar.CTL_FIELDS:
        want = min(cb[k], cb["steps_taken"]) if k == "target_steps" else cb[k]  # (resting = the target taken back to the steps held)
        assert ca[k] == want, (tag, "a resting member's control block moved", k, ca[k], want)
    for a, b, what in zip(parts_after, parts_before, ("A.part", "At.part")):
        assert ar.bits_equal(a, b), (tag, "a resting member's partial sums moved", what)


def batch_attempt(batch, devs, S, probs, sp, tag, worst, on=None, jag=(False, False)):
    """ONE lockstep attempt through the hook; every member with on[l] checked against the state IT held in front of the attempt, every
    other member (and every member whose error is up) asserted untouched -> the K results (None for a resting member)"""
    K = len(devs)
    on = [1] * K if on is None else list(on)
    if not hasattr(worst, "bits"):
        worst.bits = collections.Counter()
    before = [sc.snapshot(d) for d in devs]
    parts = [d.parts() for d in devs]
    batch.debug_attempts(1, on)
    after = [sc.snapshot(d) for d in devs]
    va, vt = batch.view(0), batch.view(1)
    assert va["vK"].shape == (S.n, K) and vt["vK"].shape == (S.m, K), (tag, va["vK"].shape, vt["vK"].shape)
    out = []
    for l in range(K):
        who = "%s LP %d" % (tag, l)
        xk, yk = va["vK"][:, l], vt["vK"][:, l]
        if not on[l] or before[l]["ctl"]["error"]:
            _untouched(who, before[l], after[l], parts[l], devs[l].parts())
            assert ar.bits_equal(xk, np.zeros(S.n)), (who, "a resting member's entries of xK are not +0.0", ar._first(xk, np.zeros(S.n)))
            out.append(None)
            continue
        after[l]["XBAR"] = xk.copy()  # (the batch keeps xbar in the interleaved vector only: check_attempt compares it with the reference's bits)
        r = ar.check_attempt(S, probs[l], sp, before[l], after[l], who)
        flipped = after[l]["ctl"]["cur"] != before[l]["ctl"]["cur"]
        y_new, aty_new = (after[l]["Y"], after[l]["ATY"]) if flipped else (after[l]["Y_OTHER"], after[l]["ATY_OTHER"])
        t = left_to_right(S, probs[l], before[l]["ctl"], before[l])
        if not (jag[0] or jag[1]):
            assert ar.bits_equal(y_new, t["y"]), (who, "y' is not the left-to-right row sum's", ar._first(y_new, t["y"]))
            assert ar.bits_equal(aty_new, t["aty"]), (who, "A^T y' is not the left-to-right row sum's", ar._first(aty_new, t["aty"]))
            assert ar.bits_equal(yk, t["y"]), (who, "yK does not hold y'", ar._first(yk, t["y"]))
        else:  # (the derived bounds are the pass condition there; how the bits compare with the left-to-right sums is REPORTED)
            assert ar.bits_equal(yk, y_new), (who, "yK does not hold y'", ar._first(yk, y_new))
            aty_from_own_y = ar.rowsums_f64(probs[l]["AT_VALUES"], y_new, S.t_off, S.t_rows)  # (so that a bit of y' does not count twice)
            for what, got, ref in (("y", y_new, t["y"]), ("aty", aty_new, aty_from_own_y)):
                differs = got.view(np.int64) != ref.view(np.int64)
                worst.bits[what + " entries"] += len(got)
                worst.bits[what + " differ"] += int(differs.sum())
                worst.bits[what + " differ in the sign of zero only"] += int((differs & (got == 0.0) & (ref == 0.0)).sum())
        assert (aty_new[S.len_c == 0] == 0.0).all(), (who, "A^T y' of an empty column")
        assert not np.signbit(aty_new[S.len_c == 0]).any(), (who, "A^T y' of an empty column is -0.0")
        worst.take(r["ratios"])
        out.append(r)
    return out


def run_batch_scenario(batch, devs, S, probs, sp, name, refresh=None, jag=(False, False)):
    """The five steps of tests/test_batch_attempts_gpu.py's docstring on K members behind one batch.  devs[l]: attempt_scenario's
    interface over member l plus parts() -> (A.part, At.part) and free_rows() (step 5: the member reset to free rows and to the start
    of attempt_scenario.tiny_lp's fixed-point kind).  refresh(l) -> member l's scaled problem after that reset.  -> Worst"""
    K, worst = len(devs), sc.Worst()
    worst.bits = collections.Counter()  # (jagged sides: entries of y' and A^T y' whose bits are not the left-to-right sums')
    # 1. eight natural attempts, all members on
    seen = [[] for _ in range(K)]
    for i in range(sc.NATURAL_ATTEMPTS):
        for l, r in enumerate(batch_attempt(batch, devs, S, probs, sp, "%s attempt %d" % (name, i), worst, jag=jag)):
            sc.assert_decided(r, "%s attempt %d LP %d" % (name, i, l))
            seen[l].append(r)
    for l in range(K):
        assert {r["cur_before"] for r in seen[l] if r["accepted"]} == {0, 1}, (name, l, "accepted from both sides of the ping-pong pairs")
        assert {r["pending_before"] for r in seen[l]} == {0, 1}, (name, l, "attempts with and without a pending average")
    # 2. member 1 alone is forced into a rejection: rejected and accepted members in ONE launch, cur parities differ afterwards
    held = sc.check_flush(devs[1], name + " flush LP 1")
    y_kept = sc.force_rejection(devs[1], S, probs[1], sp, held, name)
    rs = batch_attempt(batch, devs, S, probs, sp, name + " forced rejection", worst, jag=jag)
    assert not rs[1]["accepted"] and rs[1]["margin"] >= sc.FORCED_MARGIN, (name, "the forced rejection", rs[1])
    assert all(r["accepted"] for l, r in enumerate(rs) if l != 1), (name, "the other members next to the forced rejection", rs)
    devs[1].put("Y", y_kept)
    # 3. the running sums flushed on some members only: pending_avg differs between the members of one launch
    for l in ([0, 2] if K > 2 else [1]):
        sc.check_flush(devs[l], "%s flush LP %d" % (name, l))
    rs = batch_attempt(batch, devs, S, probs, sp, name + " mixed pending", worst, jag=jag)
    assert {r["pending_before"] for r in rs} == {0, 1}, (name, "pending_avg does not differ between the members", rs)
    # 4. half of the members rest
    on = [1 - l % 2 for l in range(K)]
    rs = batch_attempt(batch, devs, S, probs, sp, name + " half resting", worst, on=on, jag=jag)
    assert [r is not None for r in rs] == [bool(v) for v in on]
    # 5. the last member at a fixed point (free rows, zero gradient, y = 0): the step error for it alone, then its buffers freeze
    e = K - 1
    devs[e].free_rows()
    if refresh is not None:
        probs[e] = refresh(e)
    before = sc.snapshot(devs[e])
    rs = batch_attempt(batch, devs, S, probs, sp, name + " fixed point", worst, jag=jag)
    sc.assert_scalar_branch("fixed-point", rs[e], before, sc.snapshot(devs[e]), sp)
    assert all(r["error"] == 0 for l, r in enumerate(rs) if l != e), (name, rs)
    rs = batch_attempt(batch, devs, S, probs, sp, name + " behind the step error", worst, jag=jag)
    assert rs[e] is None and all(r is not None and r["error"] == 0 for l, r in enumerate(rs) if l != e), (name, rs)
    return worst


# ---- K float64 stand-ins behind the batch's interface ----------------------------------------------------------------------------------------
class Member(sc.HostStandIn):
    """attempt_scenario.HostStandIn as a member of a multi-launch batch: a rejected trial iterate is written to the other side, every row
    and column is summed left to right.  It stands in for the device; it is no second reference."""

    def __init__(self, S, prob, sp, x, y):
        super().__init__(S, prob, sp, x, y)
        self.part = (np.zeros(1), np.zeros(2))
        self.y_trial = np.zeros(S.m)

    def row_sums(self, xbar):
        return ar.rowsums_f64(self.prob["A_VALUES"], xbar, self.S.off, self.S.idx)

    def _at(self, y):
        return ar.rowsums_f64(self.prob["AT_VALUES"], y, self.S.t_off, self.S.t_rows)

    def parts(self):
        return self.part[0].copy(), self.part[1].copy()

    def _attempt(self):
        c, P, v = self.c, self.prob, self.v
        if c["error"] or c["steps_taken"] >= c["target_steps"]:
            return False
        cur = c["cur"]
        x, y, aty = self.x[cur], self.y[cur], self.aty[cur]
        nxt = x - c["tau"] * (P["C"] - aty)
        nxt = np.where(nxt < P["UB"], nxt, P["UB"])
        nxt = np.where(nxt > P["LB"], nxt, P["LB"])
        v["XBAR"] = nxt - x + nxt
        ny = y - c["sigma"] * self.row_sums(v["XBAR"])
        with np.errstate(invalid="ignore"):
            low, up = ny + c["sigma"] * P["LO"], ny + c["sigma"] * P["HI"]
        inner = np.where(up < 0.0, up, 0.0)
        ny = np.where(low > inner, low, inner)
        if c["pending_avg"]:
            v["SUM_X"], v["SUM_Y"] = v["SUM_X"] + c["step_size"] * x, v["SUM_Y"] + c["step_size"] * y
        naty = self._at(ny)
        dx, dy = nxt - x, ny - y
        sums = float(np.sum(dy * dy)), float(np.sum((naty - aty) * dx)), float(np.sum(dx * dx))
        self.c = ar.decision(c, *sums, self.sp)["ctl"]
        self.x[cur ^ 1], self.y[cur ^ 1], self.aty[cur ^ 1] = nxt, ny, naty
        self.part, self.y_trial = (np.array(sums[:1]), np.array(sums[1:])), ny
        return True

    def free_rows(self):
        """the start of attempt_scenario.tiny_lp's fixed-point kind on this matrix: free rows, A^T y := c (a zero gradient), y = 0"""
        m = self.S.m
        self.prob = dict(self.prob, LO=np.full(m, -INF), HI=np.full(m, INF))
        step = self.c["step_size"]
        self.c = dict(self.c, k=0, cur=0, pending_avg=0, steps_taken=0, attempts=0, target_steps=0, error=0, its_since_restart=0, sum_weights=0.0,
                      last_interaction=0.0, last_movement=0.0, last_dx2=0.0, last_dy2=0.0)
        self.y, self.aty = [np.zeros(m), np.zeros(m)], [self.prob["C"].copy(), np.zeros(self.S.n)]
        self.v["SUM_X"], self.v["SUM_Y"] = np.zeros(self.S.n), np.zeros(m)
        self.set_step(step, 1.0)


class BatchStandIn:
    """K Members over one matrix behind SharedMatrixBatch's debug_attempts / view"""

    def __init__(self, devs, row0_a, row0_t, layout="stream"):
        self.devs, self.row0, self.layout = list(devs), (np.asarray(row0_a), np.asarray(row0_t)), layout
        S, K = devs[0].S, len(devs)
        self.xK, self.yK = np.zeros((S.n, K)), np.zeros((S.m, K))

    def debug_attempts(self, count=1, on=None):
        K = len(self.devs)
        on = [1] * K if on is None else on
        for l, d in enumerate(self.devs):
            d.c["target_steps"] = d.c["steps_taken"] + count if on[l] and not d.c["error"] else min(d.c["target_steps"], d.c["steps_taken"])
        for _ in range(count):
            for l, d in enumerate(self.devs):
                if d._attempt():
                    self.xK[:, l], self.yK[:, l] = d.v["XBAR"], d.y_trial
                else:
                    self.rest(l)
        return [d.ctl() for d in self.devs]

    def rest(self, l):
        self.xK[:, l] = 0.0

    def view(self, side):
        S, K = self.devs[0].S, len(self.devs)
        return dict(K=K, W=len(self.row0[side]) - 1, layout=self.layout, rows=S.n if side else S.m, row0=self.row0[side],
                    vK=(self.yK if side else self.xK).copy())


def stand_in_members(p, x0, y0, dr, dc, sp, bounds, member=None):
    """K Members prepared as tests/test_batch_attempts_gpu.py prepares the device's (attempt_scenario.stand_in's step 1 per member)
    -> (members, Structure, their scaled problems)"""
    S = ar.Structure(p["m"], p["n"], p["offsets"], p["indices"])
    a_values = np.asarray(p["values"], float) * dr[S.rows] * dc[S.idx]
    devs, probs = [], []
    for lb, ub, lo, hi, _ in bounds:
        prob = dict(A_VALUES=a_values, AT_VALUES=a_values[S.order], C=p["c"] * dc, LB=lb / dc, UB=ub / dc, LO=lo * dr, HI=hi * dr)
        x = np.asarray(x0, float) / dc
        d = (member or Member)(S, prob, sp, np.minimum(np.maximum(x, prob["LB"]), prob["UB"]), np.asarray(y0, float) / dr)
        d.dr, d.dc = dr, dc
        d.set_step(1.0 / np.abs(a_values).max(), 1.0)
        d.compute_aty()
        devs.append(d)
        probs.append(prob)
    return devs, S, probs
