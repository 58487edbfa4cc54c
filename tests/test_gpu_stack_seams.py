"""The seams of the ordered batch add (``_add_batch`` in pyprobables_amd/expandingbloom.py): every case of
tests/golden/golden_stack_seams.json -- streams of CHOSEN bit positions recorded from the real reference, each built to land on one cut
of a batch at a growth or rotation -- through ExpandingBloomFilter / RotatingBloomFilter as one batch, key by key, and cut in two at every
position; then one longer stream against tests/stack_model.py.  A hash is the bit position itself.  All comparisons are exact."""

import json
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import stack_model as M  # noqa: E402

CASES = json.loads((ROOT / "tests" / "golden" / "golden_stack_seams.json").read_text())["cases"]
IDS = [c["name"] for c in CASES]


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def pa(torch):
    import pyprobables_amd

    return pyprobables_amd


def parse(op):
    if op in ("push", "pop"):
        return op, None
    return op[0], [int(x) for x in op[1:].split(".")]


def runs_of(ops):
    """maximal runs of adds of one kind -- what a caller hands over as one batch: (first op, one past the last, kind)"""
    out, i = [], 0
    while i < len(ops):
        j = i + 1
        while ops[i][0] in "af" and j < len(ops) and ops[j][0] == ops[i][0]:
            j += 1
        out.append((i, j, ops[i][0]))
        i = j
    return out


def make(pa, case):
    if case["load"] is not None:
        blm = pa.RotatingBloomFilter.frombytes(bytes.fromhex(case["load"]), max_queue_size=case["queue"])
    elif case["kind"] == "rbf":
        blm = pa.RotatingBloomFilter(est_elements=case["est_elements"], false_positive_rate=case["fpr"], max_queue_size=case["queue"])
    else:
        blm = pa.ExpandingBloomFilter(est_elements=case["est_elements"], false_positive_rate=case["fpr"])
    assert (blm._blooms[0].number_bits, blm._blooms[0].number_hashes) == (case["m"], case["k"])
    return blm


def state(blm):
    return [len(blm._blooms), [b.elements_added for b in blm._blooms], blm.elements_added]


def replay(pa, case, cuts_of):
    """the whole case with every run of adds cut at the positions ``cuts_of(run number, length)`` gives; the state is compared with the
    fixture after every batch, the export and the recorded answers at the end"""
    ops = [parse(op) for op in case["ops"]]
    blm = make(pa, case)
    for r, (lo, hi, kind) in enumerate(runs_of(ops)):
        if kind not in "af":
            getattr(blm, kind)()
            assert state(blm) == case["trace"][lo]
            continue
        edges = [0] + sorted(cuts_of(r, hi - lo)) + [hi - lo]
        for a, b in zip(edges, edges[1:]):
            keys = [bits for _, bits in ops[lo + a:lo + b]]
            if len(keys) == 1:
                blm.add_alt(keys[0], kind == "f")
            else:
                blm.add_alt_many(keys, force=kind == "f")
            assert state(blm) == case["trace"][lo + b - 1], (case["name"], r, a, b)
    assert bytes(blm).hex() == case["hex"]
    probes = case["check"]["used"] + case["check"]["unused"]
    got = blm.check_alt_many([bits for bits, _ in probes])
    assert [bool(x) for x in got] == [want for _, want in probes]
    assert [blm.check_alt(bits) for bits, _ in probes[:3]] == [want for _, want in probes[:3]]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_run_of_adds_as_one_batch(pa, case):
    replay(pa, case, lambda r, n: [])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_key_by_key(pa, case):
    replay(pa, case, lambda r, n: list(range(1, n)))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cut_in_two_at_every_position(pa, case):
    ops = [parse(op) for op in case["ops"]]
    tried = 0
    for r, (lo, hi, kind) in enumerate(runs_of(ops)):
        for cut in range(1, hi - lo if kind in "af" else 0):
            replay(pa, case, lambda rr, n, r=r, cut=cut: [cut] if rr == r else [])
            tried += 1
    assert tried == sum(hi - lo - 1 for lo, hi, kind in runs_of(ops) if kind in "af") > 0


# ---------------------------------------------------------------- one longer stream against the model
@pytest.mark.parametrize("queue", [None, 3], ids=["ebf", "rbf_q3"])
def test_40000_ops_over_5000_bit_sets_with_cuts_around_est_elements(pa, torch, queue):
    est, fpr = 300, 0.125
    if queue is None:
        blm = pa.ExpandingBloomFilter(est_elements=est, false_positive_rate=fpr)
    else:
        blm = pa.RotatingBloomFilter(est_elements=est, false_positive_rate=fpr, max_queue_size=queue)
    m, k = blm._blooms[0].number_bits, blm._blooms[0].number_hashes
    assert k == 3
    mod = M.StackModel(m, k, est, queue, blm.false_positive_rate)
    rng = np.random.default_rng(300 + (queue or 0))
    pool = rng.integers(0, m, size=(5000, k), dtype=np.int64)
    pool[::97, 1] = pool[::97, 0]  # some keys name a bit twice
    seq = rng.integers(0, 5000, size=40_000)
    seq[20_000:30_000] = seq[10_000:20_000]  # a long stretch of repeats
    p, batches = 0, 0
    while p < len(seq):
        step = min(int(rng.choice([1, 2, 299, 300, 301, 9000])), len(seq) - p)
        force = bool(rng.integers(0, 8) == 0) and step <= 301
        hashes = np.ascontiguousarray(pool[seq[p:p + step]])
        if batches % 2:
            blm.add_alt_many(torch.from_numpy(hashes).cuda(), force=force)
        else:
            blm.add_alt_many(hashes.view(np.uint64), force=force)
        for row in hashes.tolist():
            mod.add_alt(row, force)
        p += step
        batches += 1
        assert state(blm) == [len(mod.filters), mod.counts(), mod.elements_added], (batches, p, step, force)
    assert bytes(blm) == mod.export()
    probes = np.concatenate([pool, rng.integers(0, m, size=(2000, k), dtype=np.int64)])
    got = blm.check_alt_many(torch.from_numpy(probes).cuda()).cpu().numpy()
    assert got.astype(np.uint8).tolist() == [int(mod.check_alt(row)) for row in probes.tolist()]
    assert len(mod.filters) > 2
