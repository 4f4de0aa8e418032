"""What the NMS cases of tests/_nms_cases.py reach, proved on the host (no GPU).

dodt_nms is structure more than arithmetic: counted ranks or a bitonic sort, row chunks planned on the host, 64-row
blocks resolved as a fixed point, a `removed` vector handed from chunk to chunk.  This file asserts

  * on the plans of dodt_nms_plan_host, that the case table takes every branch of the chunk plan, both sides of the
    ranked / bitonic edge, sorts of 8 and of 16 tiles and a hand-over sweep of several trips;
  * that every construction's keep list is the oracle's;
  * with tests/_nms_model.py, that the kernel's structure without defects gives the oracle's list on every case, and
    that each defect of the model changes the list of at least one case -- so a case removed that alone reached a
    branch or caught a defect fails here first.

tests/test_gpu_nms.py runs the same cases on the device.  `PYTHONPATH=. python tests/test_nms_cases.py` prints which cases of
tests/test_gpu_ops.py::test_nms_matches_oracle catch which defect (a report, nothing is asserted on it)."""
import numpy as np
import pytest

import _nms_cases as nc
import _nms_model as nm
from dodt_amd import ops
from oracle import tfops

F32 = np.float32


def _table_plans():
    """(id, n, k, plan) of every device call the table makes."""
    out = []
    for c in list(nc.constructed_cases()) + list(nc.count_cases()):
        out.append((c.id, len(c.scores), c.k, ops.nms_plan(len(c.scores), c.k)))
    return out


def _sweep_trips(plan, n):
    """Trips of the sweep behind the first chunk when the call walks on: 64 column blocks each."""
    b1 = min((plan['chunks'][0][1] + 63) // 64, (n + 63) // 64)
    return -(-(plan['nb'] - b1) // 64) if len(plan['chunks']) > 1 else 0


def plan_branch(plan, k):
    """Which branch of the chunk plan set the first chunk."""
    by_k = -(-(k + k // 8) // 64) * 64 + 64
    if plan['n_chunks'] == 1:
        return 'single chunk'
    if plan['first_rows'] == by_k:
        return 'first chunk by max_out'
    if plan['first_rows'] == plan['later_rows']:
        return 'first chunk capped at later_rows'
    assert plan['first_rows'] == plan['n_rows'] - plan['later_rows'] and plan['n_chunks'] == 2
    return 'two chunks instead of three'


def test_plan_function_restates_the_documented_plan():
    """The plan against an independent restatement of its rules, over sizes around every edge."""
    for n in (1, 2, 63, 64, 65, 2048, 2049, 4096, 4097, 5700, 8192, 9000, 32768, 32769, 65536, 65537, 66000, 400000):
        for k in (1, 100, 300, 1024, 3641, 5000, n, n + 7):
            p = ops.nms_plan(n, k)
            nb = -(-n // 64)
            n_rows = nb * 64
            later = 4096 if nb <= 1024 else 2048
            first = min(-(-(k + k // 8) // 64) * 64 + 64, later)
            if first > n_rows or n_rows <= 2048:
                first = n_rows
            if n_rows - first > later and n_rows - later <= later:
                first = n_rows - later
            chunks, row0 = [], 0
            while row0 < n_rows:
                rows = min(first if row0 == 0 else later, n_rows - row0)
                chunks.append((row0, rows))
                row0 += rows
            n_pad = 2
            while n_pad < n:
                n_pad *= 2
            assert (p['nb'], p['n_rows'], p['n_pad']) == (nb, n_rows, n_pad)
            assert p['ranked'] == (n <= 32768) and p['sort_tiles'] == (0 if n <= 32768 else n_pad // 8192)
            assert (p['first_rows'], p['later_rows'], p['chunks']) == (first, later, chunks), (n, k)
            assert p['n_chunks'] == len(chunks) and p['chunk_rows'] == min(n_rows, later)
            assert sum(r for _, r in chunks) == n_rows and all(r % 64 == 0 and 0 < r <= 4096 for _, r in chunks)
            assert p['scan_lds_bytes'] == 8 * (nb + p['chunk_rows'] + p['chunk_rows'] // 64) <= 128 * 1024
            assert p['scratch_bytes'] >= 8 * p['chunk_rows'] * nb + 8 * n_pad + 20 * n_rows
    assert ops.nms_plan(0, 5)['n_chunks'] == 0 and ops.nms_plan(5, 0)['chunks'] == []
    with pytest.raises(ValueError):
        ops.nms_plan(400001, 5)
    with pytest.raises(ValueError):
        ops.nms_plan(-1, 5)


def test_bench_shapes_keep_their_chunks():
    """The RPN's 5760 rows at k = 1024 run as 1664 + 4096 rows, NMS #2 (P = 1024 rows, k = 100) as one chunk; the dense
    scene (BASELINE.json configs[4]: 13 085 anchors -> 4096 proposals -> 100) as four chunks and two."""
    assert ops.nms_plan(5760, 1024)['chunks'] == [(0, 1664), (1664, 4096)]
    assert ops.nms_plan(5700, 1024)['chunks'] == [(0, 1664), (1664, 4096)]
    assert ops.nms_plan(1024, 100)['chunks'] == [(0, 1024)]
    assert ops.nms_plan(300, 100)['chunks'] == [(0, 320)]
    assert ops.nms_plan(13085, 4096)['chunks'] == [(0, 4096), (4096, 4096), (8192, 4096), (12288, 832)]
    assert ops.nms_plan(4096, 100)['chunks'] == [(0, 192), (192, 3904)]


def test_case_table_takes_every_plan_branch():
    plans = _table_plans()
    branches = {}
    for cid, n, k, p in plans:
        branches.setdefault(plan_branch(p, k), []).append(cid)
    assert set(branches) == {'single chunk', 'first chunk by max_out', 'first chunk capped at later_rows',
                             'two chunks instead of three'}, sorted(branches)
    by = dict((cid, (n, k, p)) for cid, n, k, p in plans)
    n, k, p = by['grid-n5700-k1024']
    assert p['n_rows'] == 5760 and p['chunks'] == [(0, 1664), (1664, 4096)]      # the RPN's own shape
    assert any(p['n_chunks'] >= 4 for _, _, _, p in plans)
    assert any(n == 66000 and p['later_rows'] == 2048 for _, n, _, p in plans)
    assert any(p['later_rows'] == 4096 and p['n_chunks'] > 1 for _, _, _, p in plans)
    assert any(n == 32768 and p['ranked'] for _, n, _, p in plans)
    assert any(n == 32769 and not p['ranked'] for _, n, _, p in plans)
    assert any(p['ranked'] and p['n_chunks'] > 2 for _, _, _, p in plans)
    assert set(p['sort_tiles'] for _, _, _, p in plans) >= {0, 8, 16}


def test_walked_cases_sweep_several_trips_and_plants_sit_on_the_seams():
    """The cases that walk past their first chunk (k = n on a planted grid) need the sweep's second trip, and have a
    plant in its first two column blocks, on every chunk's last row and on the next chunk's first."""
    for n in (9000, 66000):
        k = n
        p = ops.nms_plan(n, k)
        assert _sweep_trips(p, n) >= 2
        boxes, scores, keep, plants = nc.grid_case(n)
        rank = np.empty(n, np.int64)
        rank[tfops.nms_order(scores)] = np.arange(n)
        planted = set(rank[plants].tolist())
        b1 = p['chunks'][0][1] // 64
        assert any(r // 64 == b1 + 64 for r in planted) and any(r // 64 == b1 + 65 for r in planted)
        for row0, rows in p['chunks'][:-1]:
            assert row0 + rows - 1 in planted and row0 + rows in planted
        assert n - 1 in planted and 0 not in planted
        # a full first chunk: its last row is 63 column blocks behind the top box's block
        assert p['chunks'][0] == (0, 4096) or n != 9000
    # chains: the longest chain inside a block is the block
    b, s, keep = nc.chain(128, 0)
    rank = np.empty(128, np.int64)
    rank[tfops.nms_order(s)] = np.arange(128)
    assert np.array_equal(np.sort(rank[keep]), np.arange(0, 128, 2))
    b, s, keep = nc.chain(128, 1)
    rank[tfops.nms_order(s)] = np.arange(128)
    assert np.array_equal(np.sort(rank[keep]), np.concatenate([[0], np.arange(1, 128, 2)]))


def test_exact_threshold_pairs_are_exact_in_the_oracle_arithmetic():
    """Each pair's float32 IoU, by the oracle's operations, equals its float32 threshold bit for bit -- the pairs
    for the pipeline's own thresholds 0.8 and 0.01 included -- so `>` flips exactly at the next float below."""
    def iou(bi, bj):
        area_i = F32(bi[2] - bi[0]) * F32(bi[3] - bi[1])
        area_j = F32(bj[2] - bj[0]) * F32(bj[3] - bj[1])
        iy = max(F32(min(bi[2], bj[2]) - max(bi[0], bj[0])), F32(0))
        ix = max(F32(min(bi[3], bj[3]) - max(bi[1], bj[1])), F32(0))
        inter = F32(iy * ix)
        return F32(inter / F32(F32(area_i + area_j) - inter))
    seen = set()
    for name, b, s, thr, keep in nc.exact_threshold():
        pairs = [(i, j) for i in range(len(b)) for j in range(i + 1, len(b))]
        if 'below' in name:
            at = F32(np.nextafter(thr, F32(1)))
            assert thr < at, name
            assert any(tfops._iou_gt(b[i], b[j], thr) and not tfops._iou_gt(b[i], b[j], at) for i, j in pairs), name
            continue
        exact = [(i, j) for i, j in pairs if iou(b[i], b[j]).tobytes() == F32(thr).tobytes()]
        assert exact and not any(tfops._iou_gt(b[i], b[j], thr) for i, j in exact), name
        seen.add(float(thr))
    assert seen == {0.5, 0.25, float(F32(0.8)), float(F32(0.01))}


def test_poison_leaves_the_valid_rows_alone():
    b, s = nc.count_base(130)
    pb, ps = nc.poison(b, s, 65)
    assert np.array_equal(pb[:65], b[:65]) and np.array_equal(ps[:65], s[:65])
    assert np.isinf(ps[65]) and np.isnan(ps[66]) and np.isnan(pb[65]).all() and abs(pb[66]).min() == F32(1e30)
    pb, ps = nc.poison(b, s, 1130)
    assert np.array_equal(pb, b) and np.array_equal(ps, s)


def _oracle(c, limit=20000):
    n = len(c.scores)
    n_eff = n if c.n_eff is None else min(c.n_eff, n)
    if n > limit and c.k > 3000:
        return None         # with everything kept the oracle takes minutes: the construction's list stands alone
    return tfops.non_max_suppression_fast(c.boxes[:n_eff], c.scores[:n_eff], c.k, c.thr)


@pytest.mark.parametrize('gen', [nc.chain_cases, nc.grid_cases, nc.threshold_cases, nc.tie_cases],
                         ids=lambda g: g.__name__)
def test_constructions_match_the_oracle(gen):
    checked = 0
    for c in gen():
        assert c.keep.dtype == np.int32 and len(c.keep) <= c.k
        want = _oracle(c)
        if want is None:
            assert c.id == 'grid-n66000-k66000'
            continue
        assert np.array_equal(c.keep, want), c.id
        checked += 1
    assert checked


def test_small_constructions_match_the_plain_oracle():
    """Two small sizes against the pure-python loop, which shares no code with the vectorised twin."""
    for n, lead in ((65, 0), (128, 1)):
        b, s, keep = nc.chain(n, lead)
        assert np.array_equal(keep, tfops.non_max_suppression(b, s, n, F32(0.5)))
    for n in (130, 700):
        b, s, keep, plants = nc.grid_with_plants(n, [1, 63, 64, 65, n - 1], seed=n)
        assert np.array_equal(keep, tfops.non_max_suppression(b, s, n, F32(0.5)))
        assert not set(plants.tolist()) & set(keep.tolist())
    b, s, keep = nc.ties(300)
    assert np.array_equal(keep, tfops.non_max_suppression(b, s, 300, F32(0.5)))
    for c in list(nc.threshold_cases()) + [next(nc.tie_cases())]:
        assert np.array_equal(c.keep, tfops.non_max_suppression(c.boxes, c.scores, c.k, c.thr)), c.id


def test_model_iou_is_the_oracles():
    rng = np.random.default_rng(5)
    b, _ = nc.random_boxes(rng, 400, 0.2)
    b[::7] = b[::7][:, [2, 3, 0, 1]]
    b[::11, 2] = b[::11, 0]
    i, j = rng.integers(0, 400, 3000), rng.integers(0, 400, 3000)
    for thr in (F32(0.3), F32(0.01)):
        want = np.array([tfops._iou_gt(b[a], b[c], thr) for a, c in zip(i, j)])
        assert np.array_equal(nm.iou_gt(b[i], b[j], thr), want) and want.any() and not want.all()


# ---- the model of the structure ---------------------------------------------------------------------------------

MODEL_COUNT_SIZES = (130, 2049, 9000)       # the poisoned cases the model walks (40 000 adds no structure to them)


def model_cases():
    for c in nc.constructed_cases():
        yield c
    for c in nc.count_cases(MODEL_COUNT_SIZES):
        yield c


_SORTED = {}


def _sorted(c, **kw):
    """The case in candidate order with its hits, shared by the cases that differ in k alone."""
    key = (c.id.rsplit('-k', 1)[0] if c.n_eff is None else c.id, float(c.thr), tuple(sorted(kw.items())))
    if key not in _SORTED:
        _SORTED[key] = nm.Sorted(c.boxes, c.scores, c.thr, c.n_eff, **kw)
    return _SORTED[key]


def model_keep(c, defect=None):
    kw = {}
    if defect == 'pads_unmasked':
        if c.n_eff is None or c.n_eff >= len(c.scores) or len(c.scores) > 2049:
            return model_keep(c)        # nothing to unmask (or too many all-covering pad boxes to pair up)
        kw['pads_unmasked'] = True
    if defect == 'neg_zero_below':
        if not (np.signbit(c.scores) & (c.scores == 0)).any():
            return model_keep(c)
        kw['neg_zero_below'] = True
    return nm.run(_sorted(c, **kw), ops.nms_plan(len(c.scores), c.k), c.k, defect)


_WANT = {}


def _want(c):
    """The construction's list; the oracle's (computed once) where a case has none."""
    if c.keep is not None:
        return c.keep
    if c.id not in _WANT:
        _WANT[c.id] = _oracle(c)
    return _WANT[c.id]


def test_model_without_defects_is_the_oracle():
    for c in model_cases():
        # (a constructed case's own list is the oracle's: test_constructions_match_the_oracle)
        assert np.array_equal(model_keep(c), _want(c)), c.id


def defect_table(cases, want):
    """defect -> ids of the cases whose keep list it changes."""
    return dict((d, [c.id for c in cases if not np.array_equal(model_keep(c, d), want(c))]) for d in nm.DEFECTS)


def test_every_defect_changes_a_case():
    caught = defect_table(list(model_cases()), _want)
    for d in nm.DEFECTS:
        assert caught[d], 'no case of the table notices the defect %r' % d
    # the cases built for a defect catch it
    assert 'chain-n64-lead0-k33' in caught['fixed_point_8']
    assert 'chain-n4500-lead1-k5000' in caught['no_sweep'] and 'grid-n9000-k9000' in caught['no_sweep']
    assert 'grid-n9000-k9000' in caught['sweep_one_trip'] and 'grid-n66000-k66000' in caught['sweep_one_trip']
    assert 'grid-n9000-k9000' in caught['reach_short']
    assert 'zeros-tiny' in caught['neg_zero_below'] and 'ties-n33000-k500' in caught['neg_zero_below']
    assert 'chain-n64-lead0-k1' in caught['no_room_cut']
    assert any(i.startswith('count-n2049') for i in caught['pads_unmasked'])


# ---- report: what the existing random cases would have caught ----------------------------------------------------

EXISTING = [(1, 10, 0.5, 0.1), (2, 1, 0.5, 0.1), (63, 100, 0.5, 0.2), (64, 64, 0.3, 0.2), (65, 1000, 0.8, 0.2),
            (1000, 100, 0.01, 0.05), (2048, 300, 0.8, 0.1), (2049, 1024, 0.8, 0.1), (4100, 1024, 0.5, 0.05),
            (8192, 1024, 0.8, 0.03), (9000, 300, 0.8, 0.03), (14000, 1024, 0.8, 0.03), (20000, 2000, 0.6, 0.02),
            (16000, 1024, 0.3, 0.1), (40000, 700, 0.7, 0.015)]      # test_gpu_ops.py::test_nms_matches_oracle


def existing_cases():
    for n, k, thr, scale in EXISTING:
        b, s = nc.random_boxes(np.random.default_rng(n * 31 + k), n, scale)
        k = min(k, n)           # tf_image.non_max_suppression clamps
        yield nc.Case('existing-n%d-k%d' % (n, k), b, s, k, F32(thr), None,
                      tfops.non_max_suppression_fast(b, s, k, F32(thr)))


if __name__ == '__main__':
    new = defect_table(list(model_cases()), _want)
    old_cases = list(existing_cases())
    for c in old_cases:
        assert np.array_equal(model_keep(c), c.keep), c.id
    old = defect_table(old_cases, lambda c: c.keep)
    for d in nm.DEFECTS:
        print('%-16s new: %3d cases (e.g. %s)   existing: %s' % (d, len(new[d]), ', '.join(new[d][:3]),
                                                                ', '.join(old[d]) or 'none'))
    for cid, n, k, p in _table_plans():
        if not cid.startswith('count') or 'thr0.8' in cid and 'neff0-' in cid:
            print('%-28s %-34s chunks %2d  %s  sweep trips %d' % (
                cid, plan_branch(p, k), p['n_chunks'], 'ranked' if p['ranked'] else 'bitonic %d tiles' % p['sort_tiles'],
                _sweep_trips(p, n)))
