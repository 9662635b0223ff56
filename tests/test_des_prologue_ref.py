"""CPU: the numpy references of tests/des_prologue_ref.py pinned to the oracle (oracle/des_prologue.py, itself pinned
to the upstream code by tests/golden/des_prologue.npz), and the case tables checked to reach what they claim: the
inputs the GPU file (test_des_prologue_edges_gpu.py) uses tell every planted reference fault from the real thing."""
import numpy as np
import pytest

import des_prologue_ref as R
from oracle import des_prologue as odp

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _run_oracle(form, S, m, g2, monkeypatch):
    """The oracle under a seed with ``np.random.choice`` recorded (its stream undisturbed) -> per sample
    (spec, sources drawn or None, residue columns)."""
    real, calls, per_sample = np.random.choice, [], []

    def recording(a, size=None, replace=True, p=None):
        got = real(a, size=size, replace=replace, p=p)
        calls.append((size is not None, got))
        return got

    def on_spec(spec):
        drawn = [np.asarray(c) for s_, c in calls if s_]
        per_sample.append((spec, drawn[0] if drawn else None, np.array([int(c) for s_, c in calls if not s_])))
        calls.clear()

    monkeypatch.setattr(np.random, "choice", recording)
    np.random.seed(40 + S)
    if form == "midi":
        odp.midi_prologue(m[:, None], g2, adj_size=(S, S), instrument=None, on_spec=on_spec)
    else:
        odp.wav_prologue(m, size=S, on_spec=on_spec)
    pos = np.random.randint(0, 2 ** 31 - 1)
    monkeypatch.setattr(np.random, "choice", real)
    # the wrapper left the stream alone: the same call without it ends at the same position
    np.random.seed(40 + S)
    if form == "midi":
        odp.midi_prologue(m[:, None], g2, adj_size=(S, S), instrument=None)
    else:
        odp.wav_prologue(m, size=S)
    assert np.random.randint(0, 2 ** 31 - 1) == pos
    return per_sample


def _check_against_oracle(form, S, m, monkeypatch):
    dim = S - (3 if form == "midi" else 5)
    args = R.SCAN_ARGS[form]
    per_sample = _run_oracle(form, S, m, R.gen2_like(len(m), S), monkeypatch)
    assert len(per_sample) == len(m)
    for b, (spec, sources, cols) in enumerate(per_sample):
        scan = R.scan_ref(m[b], S, dim, **args)
        assert scan["flag"] == 0 and len(cols) == dim
        src = np.zeros(dim, dtype=bool)
        src[sources if sources is not None else np.flatnonzero(scan["thr_mask"])] = True
        want = spec["sim_matrix"]
        assert np.array_equal(_bits(R.routing_ref(m[b], S, dim, src, cols)), _bits(want)), (form, S, b)
        assert np.array_equal(np.diag(want) == 1.0, src)
        assert scan["instruments"] == [int(x) for x in spec["instruments"]], (form, S, b)
        assert scan["note_levels"] == [int(x) for x in spec["note_levels"]], (form, S, b)
        for i in range(dim):                                      # the residue went where the zero mask allows
            assert not (scan["zero_mask"][i] >> int(cols[i])) & 1 and cols[i] != i and not src[cols[i]]
        if form == "wav":
            for i, d in enumerate(spec["distributions"]):
                k1, k2 = (30, 15) if src[i] else (5, 3)
                assert R.same_f32_bits([d[1], d[2]], [k1 * scan["aux"][0, i], k2 * scan["aux"][1, i]]), (S, b, i)


@pytest.mark.parametrize("form,S", [("midi", s) for s in R.MIDI_SIZES if s not in R.MIDI_RAISES] +
                         [("wav", s) for s in R.WAV_SIZES if s not in R.WAV_RAISES])
def test_references_equal_the_oracle_at_every_scan_size(form, S, monkeypatch):
    _check_against_oracle(form, S, R.generator_like(form, S, 4, 0), monkeypatch)


@pytest.mark.parametrize("dim", [d for d in R.ROUTING_DIMS if d > 1])
def test_references_equal_the_oracle_at_every_routing_dim(dim, monkeypatch):
    """The oracle has no size limit: the MIDI form at S = dim + 3 reaches every routing dim, 63 and 64 included."""
    _check_against_oracle("midi", dim + 3, R.generator_like("midi", dim + 3, 3, 1), monkeypatch)


def test_references_equal_the_oracle_on_the_value_edges(monkeypatch):
    """The MIDI edge sample (zeros of both signs, denormals, the k / 126 neighbours, the wrap values and 1.7e7) goes
    through the oracle whole; the wav one holds several thresholded entries, which the oracle refuses, so its rows are
    held to the oracle's statements one by one."""
    m, names = R.scan_edge_batch("midi", 64, 61)
    _check_against_oracle("midi", 64, m[[names.index("edges")]], monkeypatch)
    scan = R.scan_ref(m[0], 64, 61, **R.SCAN_ARGS["midi"])
    vals = R.int_row_values()
    assert scan["instruments"][:len(vals)] == [int(v * 126) for v in vals]
    assert scan["instruments"][len(vals) - 1] == 2142000000 and scan["flag"] == 0
    assert scan["zero_mask"][0] & 0b1111 == 0b0010 and scan["zero_mask"][1] & 1 and scan["zero_mask"][2] >> 60 == 1
    # both roundings around k / 126 and the wrap are in the table: truncation lands on k - 1 and on k, 128 wraps to 0
    got = set(scan["instruments"][:len(vals)])
    assert {0, 1, 2, 3, 6, 7, 62, 63, 99, 100, 124, 125, 126, 127, 128, 254, 255, 256} <= got
    notes = R.scan_ref(m[0], 64, 61, **R.SCAN_ARGS["midi"])["note_levels"]
    assert {0, 127} <= set(notes) and max(notes) == 127
    w, wnames = R.scan_edge_batch("wav", 64, 59)
    e = np.abs(w[wnames.index("edges")])
    ws = R.scan_ref(w[0], 64, 59, **R.SCAN_ARGS["wav"])
    assert ws["thr_mask"].tolist() == (e[59] > 0.75).astype(int).tolist()
    assert ws["thr_mask"][[0, 1, 2, 3, 63, 62]].tolist() == [0, 1, 0, 1, 1, 0] and ws["thr_mask"].sum() == 3
    assert ws["note_levels"] == [int(e[61, i] * 126) for i in range(59)] and max(ws["note_levels"]) == 2142000000
    assert R.same_f32_bits(ws["aux"][0], (e[62] / sum(e[62]))[:59]) and R.same_f32_bits(ws["aux"][1], (e[63] / sum(e[63]))[:59])


def test_the_oracle_has_no_upper_limit_and_the_reference_flags_it():
    """|m| = 1.8e7: Python's int() carries 2268000000 on; the kernel's int32 cannot, so the sample is flagged."""
    assert int(F32(1.8e7) * 126) == 2268000000
    for form, S, dim in (("midi", 64, 61), ("wav", 64, 59)):
        m, names = R.scan_edge_batch(form, S, dim)
        for b, name in enumerate(names):
            scan = R.scan_ref(m[b], S, dim, **R.SCAN_ARGS[form])
            assert scan["flag"] == int(name not in ("edges", "zero_aux", "clean")), (form, name)
        big = R.scan_ref(m[names.index("big")], S, dim, **R.SCAN_ARGS[form])
        assert big["instruments"][4] == R.INT32_SAT and big["instruments"].count(R.INT32_SAT) == 1
        note = R.scan_ref(m[names.index("big_note")], S, dim, **R.SCAN_ARGS[form])
        assert note["note_levels"][dim - 1] == (127 if form == "midi" else R.INT32_SAT)
    g1 = R.generator_like("midi", 12, 1, 0)
    g1[0, 10, 3] = 1.8e7
    np.random.seed(1)
    assert odp.midi_prologue(g1[:, None], R.gen2_like(1, 0), adj_size=(12, 12))[0]["instruments"][3] == 2268000000.0


def test_the_oracle_raises_at_the_smallest_sizes():
    for S in R.MIDI_RAISES:
        with pytest.raises(ValueError):
            np.random.seed(40 + S)
            odp.midi_prologue(R.generator_like("midi", S, 4, 0)[:, None], R.gen2_like(4, S), adj_size=(S, S))
    for S in R.WAV_RAISES:
        with pytest.raises(ValueError):
            np.random.seed(40 + S)
            odp.wav_prologue(R.generator_like("wav", S, 4, 0), size=S)


@pytest.mark.parametrize("dim,S", R.ROUTING_GEOMS)
def test_routing_table_tells_the_summation_orders_apart(dim, S):
    m, src, cols = R.routing_batch(dim, S, 4)
    assert [int(s.sum()) for s in src] == [0, 1, dim // 4, dim]
    if dim >= 3:                                                    # every kind of residue column is in the batch
        assert {-1, dim} <= set(cols.ravel().tolist()) and any(cols[k, i] == i for k in range(4) for i in range(dim))
    if dim >= 5:
        assert any(src[k, cols[k, i]] for k in (1, 2) for i in range(dim) if 0 <= cols[k, i] < dim and cols[k, i] != i)
    differ = 0
    for k in range(4):
        a = np.abs(m[k, :dim, :dim]).astype(np.float64)
        a[:, src[k]] = 0.0
        a[np.arange(dim), np.arange(dim)] = 0.0
        for row in a:
            vals = list(row)
            assert R.pairwise8(vals).hex() == row.sum().hex()               # numpy's order is the one restated here
            differ += R.pairwise8(vals).hex() != R.seq_sum(vals).hex()
        if dim >= 8 and k == 0:                                     # the constructed row, by one ulp
            vals = list(a[1])
            assert R.pairwise8(vals) == np.nextafter(R.seq_sum(vals), np.inf)
    plain = [R.routing_ref(m[k], S, dim, src[k], cols[k]) for k in range(4)]
    wrong = [R.routing_ref(m[k], S, dim, src[k], cols[k], fault="seq_sum") for k in range(4)]
    if dim >= 8:
        assert differ >= 1 and any(not np.array_equal(_bits(p), _bits(w)) for p, w in zip(plain, wrong))
    else:
        assert differ == 0 and all(np.array_equal(_bits(p), _bits(w)) for p, w in zip(plain, wrong))
    # the planted all-zero row: zero but for 1.0 at its residue column and the diagonal
    z, c = 2 % dim, (2 % dim + 1) % dim
    want = np.zeros(dim)
    want[c] = 1.0
    want[z] = 1.0 if src[1, z] else -1.0
    assert np.array_equal(_bits(plain[1][z]), _bits(want))
    assert all(np.isfinite(p).all() for p in plain)
    # every node a source: nothing but the residues and the diagonal
    assert set(np.unique(plain[3]).tolist()) <= {0.0, 1.0, 2.0}


def test_scan_tables_tell_the_planted_faults_apart():
    for form, S, dim in (("midi", 64, 61), ("wav", 64, 59)):
        m, names = R.scan_edge_batch(form, S, dim)
        e = m[names.index("edges")]
        args = R.SCAN_ARGS[form]
        good = R.scan_ref(e, S, dim, **args)
        no_abs = R.scan_ref(e, S, dim, fault="no_abs", **args)
        assert no_abs["instruments"] != good["instruments"] or no_abs["note_levels"] != good["note_levels"]
        if form == "wav":
            assert not np.array_equal(no_abs["thr_mask"], good["thr_mask"])
            assert not np.array_equal(R.scan_ref(e, S, dim, fault="ge_thr", **args)["thr_mask"], good["thr_mask"])
            wrong = R.scan_ref(e, S, dim, fault="np_sum", **args)["aux"]
            for k, row in enumerate(np.abs(e[dim + 3:dim + 5])):
                assert sum(row).tobytes() != np.sum(row).tobytes(), k         # sequential float32 against pairwise
                assert not R.same_f32_bits(wrong[k], good["aux"][k]), k
    # every generator-shaped wav batch of the table: the threshold row holds 0.8 (> only), negatives make abs matter
    for form, S, dim in R.SCAN_GEOMS:
        if dim >= 2:
            m = R.generator_like(form, S, 3, 0)
            args = R.SCAN_ARGS[form]
            good = [R.scan_ref(x, S, dim, **args) for x in m]
            bad = [R.scan_ref(x, S, dim, fault="no_abs", **args) for x in m]
            assert any(g["instruments"] != w["instruments"] or g["note_levels"] != w["note_levels"]
                       for g, w in zip(good, bad)), (form, S)


def test_zero_aux_row_gives_nan_and_nan_compares_by_class():
    m, names = R.scan_edge_batch("wav", 64, 59)
    aux = R.scan_ref(m[names.index("zero_aux")], 64, 59, **R.SCAN_ARGS["wav"])["aux"]
    assert np.isnan(aux[0]).all() and np.isfinite(aux[1]).all()
    flipped = aux.copy()
    flipped.view(np.uint32)[0] ^= 0x80000000                        # the other default NaN
    assert R.same_f32_bits(flipped, aux) and not np.array_equal(flipped.view(np.uint32), aux.view(np.uint32))
    off = aux.copy()
    off[1, 0] = np.nextafter(off[1, 0], F32(2))
    assert not R.same_f32_bits(off, aux)
    off = aux.copy()
    off[0, 5] = np.inf
    assert not R.same_f32_bits(off, aux)


def test_pack_ref_on_a_hand_written_example():
    n = [2, 0, 9]                                                   # 9 > max_records = 3: clamped
    value = np.array([1.5, 2.5, 9.0, 8.0, 8.0, 8.0, 3.5, 4.5, 5.5])
    ids = np.arange(9, dtype=np.int64)
    rec_ptr, (v, e) = R.pack_ref(n, [value, ids], 3)
    assert rec_ptr.tolist() == [0, 2, 2, 5] and v.tolist() == [1.5, 2.5, 3.5, 4.5, 5.5] and e.tolist() == [0, 1, 6, 7, 8]
    rec_ptr, (v,) = R.pack_ref([-5, 1, 3], [value], 3)
    assert rec_ptr.tolist() == [0, 0, 1, 4] and v.tolist() == [8.0, 3.5, 4.5, 5.5]
    for b, cap, pattern in R.PACK_CASES:
        n, arrays = R.pack_case(b, cap, pattern)
        assert len(n) == b and all(len(a) == b * cap for a in arrays)
        assert len(np.unique(arrays[0])) == b * cap
        if pattern == "clamped":
            assert n.min() == -5 and (b < 2 or n.max() == cap + 9)
        if pattern == "short_first":
            assert n[0] == cap - 1 == 999 and (n[1:] == 1000).all()
