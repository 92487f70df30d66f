"""What the inputs of tests/test_gpu_exact_paths.py do to the scans' selection, proved without a GPU from the replay
in tests/exact_cases.py (selection_trace, merge_model) and the reference distances alone. `cap` and `step` are the
formulae of DESIGN.md sec. 4.9 (exact_cases.cap_of, STEP), not the library's.

The last section runs variants of the selection against the same inputs. Only one of the four changes what a scan
returns, and the inputs catch it; the other three cannot change it on any input, which the tests state and check:

  merge at stride k     the lists of all slices but the first are read from the wrong place: the result differs on
                        every sliced input.
  threshold at [k]      one rank too loose. A key that passes it but not the true threshold is above k keys already
                        seen, so it is cut again: the result is the same, the kernel only appends more (the replay's
                        `appended` differs on an input made for it: the (k + 1)-th smallest key arriving last).
  trigger `>=`          compacts one step early when cap == k + step: the same result by one more sort per slice (the
                        replay's `compactions` differs).
  append at `<=`        the threshold is EMPTY or a key that has already arrived, and every key arrives once (ids are
                        unique), so no arriving key ever equals it: `<=` and `<` select the same keys on every input.
                        No input can tell them apart; the replay is identical, step for step."""
import numpy as np
import pytest

import exact_cases as E

KINDS = ("pq8", "pq", "l2")


def keys0(case, query=0):
    return E.keys_of(case["dist"][query])


def one_slice(kind, order, k, query=0, **variant):
    keys = keys0(E.order_case(kind, order), query)
    return keys, E.selection_trace(keys, k, E.cap_of(kind, k), E.STEP[kind], 0, len(keys), **variant)


# ------------------------------------------------------------------ the formulae and the orderings
def test_tight_ks_are_in_the_k_lists():
    assert E.tight_ks("pq8") == [512] and E.tight_ks("pq") == [256, 768] and E.tight_ks("l2") == [256, 768]
    assert (E.cap_of("pq8", 512), E.cap_of("pq", 256), E.cap_of("pq", 768), E.cap_of("l2", 1024)) == \
        (1024, 512, 1024, 2048)
    assert E.cap_of("pq8", 513) == 2048 and E.cap_of("pq", 257) == 1024 and E.cap_of("pq", 1) == 512
    for kind in KINDS:
        assert set(E.tight_ks(kind)) <= set(E.ORDER_KS[kind])


def test_arrange():
    d = np.array([3, 1, 2, 1, 5, 0, 2, 4], dtype=np.float32)
    ids = np.arange(8)
    assert E.arrange(ids, d, "ascending")[0].tolist() == [5, 1, 3, 2, 6, 0, 7, 4]   # ties (1, 3), (2, 6) by id
    assert E.arrange(ids, d, "descending")[0].tolist() == [4, 7, 0, 2, 6, 1, 3, 5]
    assert E.arrange(ids, d, "sawtooth", step=3)[0].tolist() == [1, 3, 5, 0, 2, 6, 4, 7]
    assert sorted(E.arrange(ids, d, "random")[0].tolist()) == list(range(8))
    for kind in KINDS:
        for order in E.ORDERS:
            c, base = E.order_case(kind, order), E.ORDER_INPUTS[kind]()
            d0 = c["dist"][0]
            assert len(d0) == E.N_ORDER and np.array_equal(np.sort(d0), np.sort(base["dist"][0]))
            if order == "ascending":
                assert (np.diff(d0) >= 0).all()
            if order == "descending":
                assert (np.diff(d0) <= 0).all()
            if order == "sawtooth":
                runs = d0.reshape(-1, E.STEP[kind])
                assert (np.diff(runs, axis=1) <= 0).all() and (runs[1:, -1] >= runs[:-1, 0]).all()


# ------------------------------------------------------------------ the replay is a scan
@pytest.mark.parametrize("kind", KINDS)
def test_replay_returns_the_k_smallest(kind):
    """Without a variant the replay of every input returns the reference, for the sorted query and an unsorted one;
    inside it asserts that no fill passes cap."""
    for order in E.ORDERS:
        c = E.order_case(kind, order)
        for k in E.ORDER_KS[kind]:
            for query in (0, 3):
                keys = keys0(c, query)
                got, _ = E.scan_model(keys, k, kind, E.N_ORDER)
                assert np.array_equal(got, E.reference_keys(keys, k)), (order, k, query)
    c = E.tie_case(kind)
    for rows in E.TIE_SLICE_ROWS + (64,):
        for k in E.tie_ks(c["dist"]) + [1, 1024]:
            for query in range(len(c["q"])):
                keys = keys0(c, query)
                got, traces = E.scan_model(keys, k, kind, rows)
                assert len(traces) == E.N_ORDER // rows
                assert np.array_equal(got, E.reference_keys(keys, k)), (rows, k, query)
    short = keys0(c)[:100]  # fewer rows than k: padded
    got, _ = E.scan_model(short, 128, kind, 64)
    assert np.array_equal(got[:100], np.sort(short)) and (got[100:] == E.EMPTY).all()


# ------------------------------------------------------------------ arrival orders
@pytest.mark.parametrize("kind", KINDS)
def test_descending_every_row_passes_and_compactions_follow(kind):
    step, steps = E.STEP[kind], E.N_ORDER // E.STEP[kind]
    for k in E.ORDER_KS[kind]:
        cap = E.cap_of(kind, k)
        _, t = one_slice(kind, "descending", k)
        assert t.passes == (step,) * steps and t.appended == E.N_ORDER  # every row of every step
        # the first compaction when cap rows have arrived, then one every `per` steps: the buffer holds k after it
        # and takes (cap - k) / step full steps
        per = (cap - k) // step
        assert t.compactions == (steps - cap // step) // per + 1 and t.first_compaction_step == cap // step - 1
        assert t.max_fill <= cap
    # the issue's figure for the tightest buffer of the tiled kernel
    _, t = one_slice("pq8", "descending", 512)
    assert t.compactions >= E.N_ORDER // 1024 - 1 and t.hit_cap and t.max_fill == 1024


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("order", ["ascending", "sawtooth"])
def test_ascending_nothing_passes_after_the_first_compaction(kind, order):
    """Rows (or runs of a step) arrive in ascending order: everything passes while the threshold is still EMPTY, the
    first compaction keeps the first k rows' keys, and no later row passes. One compaction, or none."""
    step = E.STEP[kind]
    for k in E.ORDER_KS[kind]:
        keys, t = one_slice(kind, order, k)
        assert t.compactions <= 1
        assert t.compactions == 1 and t.first_compaction_step is not None  # 8,192 rows: more than any cap
        seen = (t.first_compaction_step + 1) * step
        assert t.appended == seen and all(p == 0 for p in t.passes[t.first_compaction_step + 1:])
        assert np.array_equal(t.keys, np.sort(keys[:seen])[:k])
        assert set(t.keys.tolist()) <= set(keys[:max(k, step)].tolist())  # all from the first k rows (or first run)


@pytest.mark.parametrize("kind", KINDS)
def test_tight_k_fills_the_buffer_exactly(kind):
    """cap == k + step: after a compaction the buffer holds k, and a step in which every row passes fills it to
    exactly cap. In descending order that is every step; in every order it is the step before the first compaction."""
    for k in E.tight_ks(kind):
        cap = E.cap_of(kind, k)
        assert cap == k + E.STEP[kind]
        for order in E.ORDERS:
            _, t = one_slice(kind, order, k)
            assert t.hit_cap and t.max_fill == cap, (order, k)
        keys = keys0(E.order_case(kind, "descending"))
        fills, fill = [], 0  # the fill after each step, restated from the counts
        _, t = one_slice(kind, "descending", k)
        for p in t.passes:
            fill += p
            fills.append(fill)
            if fill + E.STEP[kind] > cap:
                fill = k
        # every step from the one that first fills the buffer on
        assert fills.count(cap) == len(fills) - (cap // E.STEP[kind] - 1) and len(keys) == E.N_ORDER


def test_random_order_compacts_a_few_times():
    """What the random inputs of the other tests do, for contrast: a handful of compactions, then almost nothing."""
    for kind in KINDS:
        _, t = one_slice(kind, "random", 128)
        _, d = one_slice(kind, "descending", 128)
        assert 1 <= t.compactions < d.compactions // 2 and t.appended < E.N_ORDER // 4


# ------------------------------------------------------------------ ties
@pytest.mark.parametrize("kind", KINDS)
def test_tie_cases_cut_inside_a_group_that_spans_slices(kind):
    c = E.tie_case(kind)
    dist = c["dist"]
    assert (np.diff(dist[0]) <= 0).all()  # descending for query 0
    for k in E.tie_ks(dist):
        srt = np.sort(dist, axis=1)
        inside = srt[:, k - 1] == srt[:, k]
        assert inside[0] and inside.sum() >= 2  # the k-th and (k + 1)-th distances are equal
        for rows in E.TIE_SLICE_ROWS:
            # some query's cut group lies in more than one slice with fewer than k nearer rows in all: which of its
            # ids are returned is decided where the slices' lists meet, in the merge
            spans = 0
            for i in np.flatnonzero(inside):
                group = np.flatnonzero(dist[i] == srt[i, k - 1])
                spans += len(np.unique(group // rows)) >= 2
            assert spans >= 1, (kind, k, rows)
    if kind != "l2":  # integer distances: the fp32 sums are exact in any order
        assert np.array_equal(dist, np.round(dist)) and dist.max() < 2 ** 24


# ------------------------------------------------------------------ variants
def _sliced_inputs():
    for kind in KINDS:
        c = E.tie_case(kind)
        for rows in E.TIE_SLICE_ROWS:
            for k in E.tie_ks(c["dist"]):
                yield kind, keys0(c), k, rows


def test_variant_merge_stride_k_is_caught():
    """The merge reading list s at ws[s * k] instead of ws[s * cap]: on every sliced input the result differs from
    the reference, even with the never-written part of the workspace holding EMPTY (the kindest garbage)."""
    n = 0
    for kind, keys, k, rows in _sliced_inputs():
        got, _ = E.scan_model(keys, k, kind, rows, merge_stride=k)
        assert not np.array_equal(got, E.reference_keys(keys, k)), (kind, k, rows)
        n += 1
    assert n == 12
    # and on the slice test's shape: 4,099 rows in slices of 64
    keys = keys0(E.l2_gauss(4099, 32))
    for k in (1, 70, 128):
        got, traces = E.scan_model(keys, k, "l2", 64, merge_stride=k)
        assert len(traces) == 65 and not np.array_equal(got, E.reference_keys(keys, k))


@pytest.mark.parametrize("kind", KINDS)
def test_variant_threshold_at_k_appends_more_and_returns_the_same(kind):
    """The two thresholds differ only for a key that falls between the k-th and the (k + 1)-th seen so far, which a
    random order produces a few times in 8,192 rows, or never. The input made for it: ascending order with the
    (k + 1)-th smallest key held back to the end. It passes the loose threshold and not the true one."""
    for k in E.ORDER_KS[kind]:
        asc, cap, step = keys0(E.order_case(kind, "ascending")), E.cap_of(kind, k), E.STEP[kind]
        late = np.concatenate([asc[:k], asc[k + 1:], asc[k:k + 1]])
        ref = E.selection_trace(late, k, cap, step, 0, len(late))
        var = E.selection_trace(late, k, cap, step, 0, len(late), thr_at_k=True)
        assert ref.passes[-1] == 0 and var.passes[-1] == 1 and var.appended == ref.appended + 1, k  # the replay differs
        assert np.array_equal(var.keys, ref.keys) and np.array_equal(ref.keys, E.reference_keys(late, k))  # not the result
        for order in E.ORDERS:
            keys, ref = one_slice(kind, order, k)
            _, var = one_slice(kind, order, k, thr_at_k=True)
            assert var.appended >= ref.appended
            assert np.array_equal(var.keys, ref.keys) and np.array_equal(ref.keys, E.reference_keys(keys, k))


@pytest.mark.parametrize("kind", KINDS)
def test_variant_trigger_ge_compacts_early_and_returns_the_same(kind):
    for k in E.tight_ks(kind):
        for order in ("descending", "random"):
            keys, ref = one_slice(kind, order, k)
            _, var = one_slice(kind, order, k, trigger_ge=True)
            assert var[:6] != ref[:6] and var.compactions > ref.compactions, (order, k)
            assert var.first_compaction_step == ref.first_compaction_step - 1
            assert np.array_equal(var.keys, ref.keys) and np.array_equal(ref.keys, E.reference_keys(keys, k))


@pytest.mark.parametrize("kind", KINDS)
def test_variant_le_is_the_same_selection(kind):
    """`<=` for `<`: no arriving key equals the threshold (see the module's docstring), so the replay is identical on
    every input here -- arrival orders and ties alike. Stated as an assertion so that a change of the keys that
    breaks their uniqueness shows up."""
    for order in E.ORDERS:
        c = E.order_case(kind, order)
        assert len(np.unique(keys0(c))) == E.N_ORDER
        for k in E.ORDER_KS[kind]:
            _, ref = one_slice(kind, order, k)
            _, var = one_slice(kind, order, k, le=True)
            assert var[:6] == ref[:6] and np.array_equal(var.buf, ref.buf)
    c = E.tie_case(kind)
    for k in E.tie_ks(c["dist"]):
        for query in range(len(c["q"])):
            keys = keys0(c, query)
            a, _ = E.scan_model(keys, k, kind, E.TIE_SLICE_ROWS[1])
            b, _ = E.scan_model(keys, k, kind, E.TIE_SLICE_ROWS[1], le=True)
            assert np.array_equal(a, b)
