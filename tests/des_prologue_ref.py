"""Plain-numpy references of the DES bridge prologue kernels (csrc/des_prologue.hip: ``gdm_des_scan``,
``gdm_des_routing``) and of the in-place compaction ``gdm_des_pack`` (csrc/des_batch.hip), with the geometry and value
tables the CPU file (test_des_prologue_ref.py) and the GPU file (test_des_prologue_edges_gpu.py) share.  No torch.

``scan_ref`` restates oracle/des_prologue.py lines 61-67 and 89-104 for ONE sample, ``routing_ref`` is
``oracle.des_prologue._routing`` statement for statement with the column ``np.random.choice`` would draw passed in;
test_des_prologue_ref.py pins both to the oracle, bit for bit, at every table size the oracle completes.

Every comparison built on these is of integers or bit patterns.  ``fault=`` plants one known mistake into a reference
(the CPU file shows that the tables' inputs tell each of them from the real thing, so a kernel making that mistake
cannot pass): "np_sum" (the aux rows summed by ``np.sum`` instead of Python's sequential ``sum()``), "no_abs",
"ge_thr" (``>=`` at the threshold) for the scan; "seq_sum" (the float64 row sums taken left to right instead of in
numpy's 8-accumulator order) for the routing.
"""
import numpy as np

F32 = np.float32
INT32_SAT = 2 ** 31 - 1      # what the kernel stores for an entry it flags (product not below 2^31, or not finite)
THRESHOLD = 0.75

# ---- tables ----------------------------------------------------------------------------------------------------------
# (form, S, dim): the MIDI form is dim = S - 3 (note_mod, no threshold, no aux), the wav form dim = S - 5 (threshold
# 0.75, aux); the last row of each form leaves unused rows between the parameter rows and the end (dim + 3 < S).
SCAN_GEOMS = tuple(("midi", s, s - 3) for s in (4, 5, 6, 7, 10, 11, 12, 19, 32, 35, 63, 64)) + (("midi", 40, 29),) + \
    tuple(("wav", s, s - 5) for s in (6, 8, 9, 12, 13, 14, 21, 24, 37, 64)) + (("wav", 33, 20),)
SCAN_ARGS = {"midi": dict(threshold=None, note_mod=True, norm_aux=False),
             "wav": dict(threshold=THRESHOLD, note_mod=False, norm_aux=True)}
# the package's own sizes: adj_size / size -> (form, S); S = 4 (MIDI) and S = 6, 7 (wav) raise ValueError upstream
MIDI_SIZES = (4, 5, 6, 7, 10, 11, 12, 19, 32, 35, 63, 64)
WAV_SIZES = (6, 7, 8, 9, 12, 13, 14, 21, 24, 37, 64)
MIDI_RAISES, WAV_RAISES = (4,), (6, 7)

ROUTING_DIMS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 29, 32, 60, 61, 63, 64)
# (dim, S): both sides of numpy's sequential / 8-accumulator switch at n = 8, tails n % 8 = 0..7, bit 63 of the row mask
ROUTING_GEOMS = tuple((d, s) for d in ROUTING_DIMS for s in (d, d + 3) if s <= 64)

# (B, max_records, pattern)
PACK_PATTERNS = ("full", "empty", "short_first", "random", "clamped")
PACK_CASES = tuple((b, {"short_first": 1000, "full": 1000, "empty": 1000, "random": 600, "clamped": 300}[p], p)
                   for b in (1, 2, 255, 256, 257, 513) for p in PACK_PATTERNS)


# ---- references ------------------------------------------------------------------------------------------------------
def seq_sum(values):
    """Left to right from 0, in the values' own type: Python's ``sum()`` / numpy's pairwise_sum below 8 elements."""
    res = type(values[0])(0) if len(values) else 0.0
    for v in values:
        res = res + v
    return res


def pairwise8(values):
    """numpy's pairwise_sum for 8 <= n <= 128: eight running sums, their tree, then the n % 8 tail."""
    n = len(values)
    if n < 8:
        return seq_sum(values)
    r = [values[j] for j in range(8)]
    i = 8
    while i < n - n % 8:
        for j in range(8):
            r[j] = r[j] + values[i + j]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for k in range(i, n):
        res = res + values[k]
    return res


def _stored_int(x):
    """``int(x * 126)`` with the float32 product and a Python int -> (value, flagged).  The oracle's value is unbounded
    (and ``int`` raises for a product that is not finite); the kernel flags the sample from 2^31 on and stores
    INT32_SAT, which is what comes back here for such an entry."""
    p = F32(x) * F32(126)
    if not np.isfinite(p) or p >= F32(2 ** 31):
        return INT32_SAT, True
    return int(p), False


def scan_ref(m, S, dim, threshold, note_mod, norm_aux, fault=None):
    """One sample m (S,S) float32 -> dict: ``thr_mask`` (S,) uint8 or None, ``instruments``, ``note_levels`` (lists of
    dim Python ints), ``zero_mask`` (dim Python ints, bit x of entry i set where |m|[i, x] == 0, x < dim), ``aux``
    (2,dim) float32 or None, ``flag`` (1 where any of the S*S entries is not finite or a converted entry is flagged)."""
    m = np.asarray(m, dtype=F32).reshape(S, S)
    with np.errstate(all="ignore"):
        a = m if fault == "no_abs" else np.abs(m)
        flag = int(not np.isfinite(m).all())
        thr_mask = None
        if threshold is not None:
            hit = a[dim] >= F32(threshold) if fault == "ge_thr" else a[dim] > F32(threshold)
            thr_mask = hit.astype(np.uint8)
        instruments, note_levels = [], []
        for i in range(dim):
            v, big = _stored_int(a[dim + 1, i])
            instruments.append(v)
            flag |= int(big)
            v, big = _stored_int(a[dim + 2, i])
            note_levels.append(max(0, v % 128) if note_mod else v)
            flag |= int(big)
        zero_mask = [int.from_bytes(np.packbits(a[i, :dim] == 0, bitorder="little").tobytes(), "little")
                     for i in range(dim)]
        aux = None
        if norm_aux:
            total = (lambda row: np.sum(row)) if fault == "np_sum" else (lambda row: sum(row))
            aux = np.stack([(a[dim + 3] / total(a[dim + 3]))[:dim], (a[dim + 4] / total(a[dim + 4]))[:dim]])
            assert aux.dtype == F32
    return {"thr_mask": thr_mask, "instruments": instruments, "note_levels": note_levels, "zero_mask": zero_mask,
            "aux": aux, "flag": flag}


def routing_ref(m, S, dim, src, cols, fault=None):
    """``oracle.des_prologue._routing`` on |m|[:dim, :dim] with ``src`` (dim,) bool in place of the index list and
    ``cols[i]`` in place of ``np.random.choice(cands)``; a column outside [0, dim) adds nothing -> (dim,dim) float64."""
    absm = np.abs(np.asarray(m, dtype=F32).reshape(S, S))
    src = np.asarray(src).astype(bool).reshape(dim)
    row_sum = (lambda row: np.float64(seq_sum(list(row)))) if fault == "seq_sum" else (lambda row: row.sum())
    sim = absm[:dim, :dim].copy()
    sim[:, src] = 0.0
    sim[np.arange(dim), np.arange(dim)] = 0.0
    sim = sim.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        if fault == "seq_sum":
            sim = sim / np.array([[row_sum(r)] for r in sim])
        else:
            sim = sim / sim.sum(axis=1, keepdims=True)
    sim[np.isnan(sim)] = 0
    for i in range(dim):
        c = int(cols[i])
        if 0 <= c < dim:
            sim[i, c] += 1 - row_sum(sim[i])
    sim[np.arange(dim), np.arange(dim)] = np.where(src, 1.0, -1.0)
    return sim


def pack_ref(n_records, arrays, max_records):
    """Counts clamped to [0, max_records], their exclusive scan, and of every array (B * max_records entries, sample b
    at b * max_records) the samples' records one after the other -> (rec_ptr (B+1,) int64, [packed arrays])."""
    n = np.clip(np.asarray(n_records, dtype=np.int64), 0, max_records)
    rec_ptr = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    packed = [np.concatenate([np.asarray(a)[b * max_records:b * max_records + n[b]] for b in range(len(n))])
              for a in arrays]
    return rec_ptr, packed


# ---- inputs ----------------------------------------------------------------------------------------------------------
def _sigmoid(r, shape):
    return (1.0 / (1.0 + np.exp(-r.standard_normal(shape)))).astype(F32)


def generator_like(form, S, b, seed):
    """(b,S,S) float32 generator-shaped matrices: sigmoid of normal, 2 % negatives, from S = 11 up 2 % exact zeros; in
    the wav form the threshold row is kept below 0.75 but for every third sample, which has one thresholded source at
    column 2 % dim (the recipe of test_des_prologue_gpu) and the sample after it, which has one at column 0 with a
    negative sign; the first instrument entry is negative in every sample.  The oracle completes on them at every table size but the
    smallest (MIDI_RAISES, WAV_RAISES)."""
    r = np.random.RandomState(7000 + 100 * S + b + (0 if form == "midi" else 50) + seed)
    m = _sigmoid(r, (b, S, S))
    if S >= 11:
        m[r.random_sample(m.shape) < 0.02] = 0.0
    m[r.random_sample(m.shape) < 0.02] *= -1.0
    if form == "wav":
        dim = S - 5
        m[:, dim, :] = np.minimum(np.abs(m[:, dim, :]), F32(0.74))
        m[::3, dim, 2 % dim] = 0.8
        m[1::3, dim, 0] = -0.8                                  # a source only through abs()
    m[:, S - 2 if form == "midi" else S - 4, 0] = -np.abs(m[:, S - 2 if form == "midi" else S - 4, 0]) - F32(0.01)
    return m


def gen2_like(b, seed):
    return _sigmoid(np.random.RandomState(900 + seed), (b, 20))


def _ulps(x):
    x = F32(x)
    return [np.nextafter(x, F32(0)), x, np.nextafter(x, F32(np.inf))]


def int_row_values():
    """Entries for the instrument / note rows: k / 126 and both float32 neighbours for several k (``int(x * 126)`` is k
    or k - 1 depending on the float32 rounding of the quotient and of the product), the same around the products
    127.99.., 128, 255 and 256 (the ``% 128`` wrap), and 1.7e7, whose product 2142000000 is the last thing below 2^31
    the tables hold.  33 values."""
    vals = []
    for k in (1, 3, 7, 63, 100, 125, 126):
        vals += _ulps(k / 126)
    for p in (128, 255, 256):
        vals += _ulps(p / 126)
    vals += [F32(127.99 / 126), F32(127.9999 / 126), F32(1.7e7)]
    return np.array(vals, dtype=F32)


def wide_row(r, n):
    """n float32 values with magnitudes 2^-20 .. 2^20 and full mantissas: any two summation orders round apart."""
    return (np.ldexp(1.0 + r.random_sample(n), r.randint(-20, 21, size=n))).astype(F32)


def order_row(r, n):
    """n >= 8 float32 values within 2^-20 .. 2^20 whose float64 sum depends on the order by construction: 2^20 at 0
    and t = 2^-20 (1 + 2^-14 + 2^-15) at 2 and 3, small integers elsewhere (position 1 is left to the diagonal).  Adding
    t to anything in [2^20, 2^21) drops its last 3/8 ulp, so left to right both are dropped, while numpy's accumulators 2
    and 3 carry the two exactly into (r2 + r3), where they make 3/4 ulp and round up."""
    row = r.randint(1, 9, size=n).astype(F32)
    row[0], row[2], row[3] = 2.0 ** 20, 2.0 ** -20 * (1 + 2.0 ** -14 + 2.0 ** -15), 2.0 ** -20 * (1 + 2.0 ** -14 + 2.0 ** -15)
    return row


def scan_edge_batch(form, S, dim):
    """The value-edge samples of part A for one geometry with dim >= 40 -> (m (B,S,S) float32, names).  Sample by name:
      edges      -0.0 / 1e-40 / smallest denormal in the routing block, the threshold row at float32(0.75) and its
                 neighbours, the integer-conversion values of ``int_row_values`` in both integer rows, the
                 summation-order aux rows
      zero_aux   aux row dim + 3 all zero (0/0 -> NaN)
      big        1.8e7 in the instrument row: flagged
      big_note   1.8e7 in the note row: flagged
      <v>@<pos>  NaN, +inf, -inf inside the routing block, in parameter row ``dim`` and in the unused corner
                 (dim + 1, S - 1); each followed by a clean sample ("clean")."""
    assert dim >= 40
    r = np.random.RandomState(31 + S + dim)
    base = generator_like(form, S, 1, 99)[0]
    names, out = [], []

    def add(name, m):
        names.append(name)
        out.append(m)

    e = base.copy()
    e[0, 1], e[0, 2], e[0, 3], e[1, 0], e[2, dim - 1] = -0.0, 1e-40, 1.4e-45, 0.0, -0.0
    e[dim - 1, dim - 1], e[dim - 1, 0] = 0.0, -1e-45
    e[dim, :] = 0.1
    t = _ulps(THRESHOLD)
    e[dim, 0], e[dim, 1], e[dim, 2], e[dim, 3], e[dim, S - 1], e[dim, S - 2] = t[1], t[2], t[0], -t[2], t[2], -t[1]
    vals = int_row_values()
    e[dim + 1, :len(vals)] = vals
    e[dim + 2, :len(vals)] = vals[::-1]
    e[dim + 2, len(vals) + 1] = -vals[-1]
    if form == "wav":
        e[dim + 3], e[dim + 4] = wide_row(r, S), wide_row(r, S)
        e[dim + 3, ::5] *= -1.0
    add("edges", e)
    if form == "wav":
        z = base.copy()
        z[dim + 3, :] = 0.0
        z[dim + 3, 1] = -0.0
        add("zero_aux", z)
    big = base.copy()
    big[dim + 1, 4] = 1.8e7
    add("big", big)
    big = base.copy()
    big[dim + 2, dim - 1] = -1.8e7
    add("big_note", big)
    for pos_name, pos in (("block", (1, 2)), ("param", (dim, 0)), ("corner", (dim + 1, S - 1))):
        for v_name, v in (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
            bad = base.copy()
            bad[pos] = v
            add(f"{v_name}@{pos_name}", bad)
            add("clean", base.copy())
    return np.stack(out).astype(F32), names


def routing_batch(dim, S, b, seed=0):
    """Part B's inputs for one geometry -> (m (b,S,S) float32, src (b,dim) bool, cols (b,dim) int32).  Sample k has
    source pattern k % 4 of (none, one, dim // 4 random, every node) and per row one residue column of the kinds
    (valid, -1, dim, the row itself, a source column), rotating with row and sample.  Sample 1 % b holds the batch's
    all-zero row (row 2 % dim, residue at a valid column).  Every sample holds one -0.0 and one denormal entry; from
    dim = 8 on row 1 of every sample is an ``order_row`` and the other odd rows hold ``wide_row`` magnitudes; where S > dim, NaN and inf stand outside the block."""
    r = np.random.RandomState(500 + 70 * dim + S + 1000 * seed + b)
    m = _sigmoid(r, (b, S, S))
    m[r.random_sample(m.shape) < 0.03] *= -1.0
    if dim >= 11:
        m[r.random_sample(m.shape) < 0.02] = 0.0
    src = np.zeros((b, dim), dtype=bool)
    cols = np.empty((b, dim), dtype=np.int32)
    for k in range(b):
        if k % 4 == 1:
            src[k, r.randint(dim)] = True
        elif k % 4 == 2:
            src[k, r.choice(dim, size=dim // 4, replace=False)] = True
        elif k % 4 == 3:
            src[k, :] = True
        if dim >= 8:
            for i in range(3, dim, 2):
                m[k, i, :dim] = wide_row(r, dim)
            m[k, 1, :dim] = order_row(r, dim)
        rows = [i for i in r.randint(dim, size=2)]
        rows = [0 if dim >= 8 and i == 1 else i for i in rows]      # not into the constructed row
        m[k, rows[0], r.randint(dim)] = -0.0
        m[k, rows[1], r.randint(dim)] = [1e-40, 1.4e-45, -1e-42][k % 3]
        if S > dim:
            m[k, dim, k % S], m[k, k % dim, dim], m[k, S - 1, S - 1] = np.nan, np.inf, -np.inf
        sources = np.flatnonzero(src[k])
        for i in range(dim):
            kind = (i + k) % 5
            valid = (i + 1 + r.randint(max(1, dim - 1))) % dim
            cols[k, i] = (valid, -1, dim, i, sources[i % len(sources)] if len(sources) else valid)[kind]
    k0, z = 1 % b, 2 % dim
    m[k0, z, :dim] = 0.0
    cols[k0, z] = (z + 1) % dim
    return m, src, cols


def pack_case(b, max_records, pattern):
    """-> (n_records (b,) int64, [value f64, event_id i64, node i32, kind i32] of b * max_records entries).  ``value``
    holds distinct doubles and ``event_id`` its own index, so a record moved to the wrong place or twice shows."""
    r = np.random.RandomState(b * 7 + max_records)
    if pattern == "full":
        n = np.full(b, max_records)
    elif pattern == "empty":
        n = np.zeros(b)
    elif pattern == "short_first":
        n = np.full(b, max_records)
        n[0] = max_records - 1
    elif pattern == "random":
        n = r.randint(0, max_records + 1, size=b)
    else:
        n = r.randint(0, max_records + 1, size=b)
        n[::3] = -5
        n[1::3] = max_records + 9
    total = b * max_records
    value = np.arange(total, dtype=np.float64) * 0.5 + 0.25
    event_id = np.arange(total, dtype=np.int64)
    node = (np.arange(total, dtype=np.int64) * 7919 % 2 ** 31).astype(np.int32)
    kind = (np.arange(total, dtype=np.int64) % 5).astype(np.int32)
    return n.astype(np.int64), [value, event_id, node, kind]


# ---- comparing ---------------------------------------------------------------------------------------------------------
def same_f32_bits(got, want):
    """Bit-equal float32 arrays, except that any NaN equals any NaN (host and device default NaNs differ in sign)."""
    g, w = np.ascontiguousarray(got, dtype=F32).view(np.uint32), np.ascontiguousarray(want, dtype=F32).view(np.uint32)
    nan = lambda u: ((u & 0x7f800000) == 0x7f800000) & ((u & 0x007fffff) != 0)             # noqa: E731
    return g.shape == w.shape and bool(np.all((g == w) | (nan(g) & nan(w))))
