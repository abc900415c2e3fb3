"""The stable LSD radix sort and the one-workgroup scan of csrc/gs_binning.hip on their own (gs_debug_sort_pairs,
gs_debug_scan_sums), launched as the depth order, the region partition, the grid encoder's slot sort and the kNN's Morton sort
launch them, against numpy's stable argsort / cumsum on the cases of tests/sort_cases.py (what each case is for:
tests/test_sort_cases_cpu.py).  Integers throughout: every comparison is exact.

Per case the workspace, the outputs, n_kept and the digit totals are filled with 0xA5 bytes first; afterwards
  * the first n outputs (depth form beyond 16 384 keys: the first n_kept) are the expected pairs,
  * n_kept and the 512 digit totals of the 9-bit form are the expected numbers,
  * output words [n, n_bound) still hold the fill - the result is read from the half the callers read, start_buf ^ (passes & 1)
    or start_buf ^ 1, so a result left in the other half shows here as well -,
  * the inputs are untouched (the depth order's keys are "kept intact, so the phase can be re-run")."""
import ctypes as C

import numpy as np
import pytest
import torch

import sort_cases as sc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
WORKSPACE_HEADROOM = 1 << 16   # bytes behind the workspace: with the key headroom of the over-count cases, no count the cases
#                                hand over can take a kernel out of an allocation, clamped or not


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "GPU test running without a GPU"
    from gsplat_amd._lib import hip_api
    return hip_api()


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(DEV)


def to_host(t):
    return t.cpu().numpy().view(np.uint32)


def filled(words):
    t = torch.empty(words, dtype=torch.int32, device=DEV)
    t.view(torch.uint8).fill_(0xA5)
    return t


def workspace(api, n_bound):
    nbytes = int(api.raw("debug_sort_tmp_bytes")(n_bound))
    assert nbytes >= 16 * n_bound
    t = torch.empty(nbytes + WORKSPACE_HEADROOM, dtype=torch.uint8, device=DEV)
    t.fill_(0xA5)
    return t


def run(api, case, tmp=None):
    """-> (rc, dict of host arrays).  tmp: a workspace to use as it is (else a freshly filled one)"""
    nb = case.n_bound
    keys = to_dev(case.keys)
    vals = to_dev(case.vals) if case.vals is not None else None
    n_dev = to_dev(np.array([case.n_dev], np.uint32))
    if tmp is None:
        tmp = workspace(api, nb)
    keys_out, vals_out, n_kept, totals = filled(nb), filled(nb), filled(1), filled(512)
    depth = case.form == "depth"
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = api.raw("debug_sort_pairs")(keys.data_ptr(), vals.data_ptr() if vals is not None else None, n_dev.data_ptr(), nb,
                                     case.end_bit, case.start_buf, case.digit_bits, 1 if depth else 0, tmp.data_ptr(),
                                     tmp.numel(), keys_out.data_ptr(), vals_out.data_ptr(), n_kept.data_ptr() if depth else None,
                                     totals.data_ptr(), st)
    torch.cuda.synchronize()
    out = dict(keys=to_host(keys_out), vals=to_host(vals_out), n_kept=int(to_host(n_kept)[0]), totals=to_host(totals),
               keys_in=to_host(keys), vals_in=to_host(vals) if vals is not None else None)
    return rc, out


def check(case, out, tail=True):
    e = sc.expected(case)
    n, m = e["n"], e["n_cmp"]
    if case.form == "depth":
        assert out["n_kept"] == e["n_kept"], ("n_kept", out["n_kept"], e["n_kept"])
    else:
        assert out["n_kept"] == sc.POISON
    for k in ("keys", "vals"):
        bad = np.flatnonzero(out[k][:m] != e[k])
        assert bad.size == 0, "%s: %s differ at %d of %d places, first at %d" % (case.name, k, bad.size, m, bad[0])
    if "totals" in e:
        assert np.array_equal(out["totals"], e["totals"]), "digit totals"
    if tail:
        assert bool((out["keys"][n:case.n_bound] == sc.POISON).all()), "keys written past the count"
        assert bool((out["vals"][n:case.n_bound] == sc.POISON).all()), "values written past the count"
    assert np.array_equal(out["keys_in"], case.keys), "the sort wrote to its key input"
    if case.vals is not None:
        assert np.array_equal(out["vals_in"], case.vals), "the sort wrote to its value input"


@pytest.mark.parametrize("name", sc.NAMES)
def test_sort_case(api, name):
    case = sc.build(name)
    rc, out = run(api, case)
    assert rc == 0
    check(case, out)


def test_nine_bit_form_refuses_ten_bits(api):
    case = sc.build("passes_9bit_e9_s0")._replace(end_bit=10)
    rc, out = run(api, case)
    assert rc == sc.GS_E_SHAPE
    assert bool((out["keys"] == sc.POISON).all()) and bool((out["vals"] == sc.POISON).all())


@pytest.mark.parametrize("name", ["count_pairs_20481", "count_depth_16384", "count_depth_16385", "count_9bit_20481", "partition_e11_s1"])
def test_a_repeated_call_gives_identical_arrays(api, name):
    case = sc.build(name)
    _, a = run(api, case)
    _, b = run(api, case)
    for k in ("keys", "vals", "totals"):
        assert np.array_equal(a[k], b[k]), k
    assert a["n_kept"] == b["n_kept"]


def widened(case, n_bound):
    """the same pairs under a larger host bound (same workspace layout as a sort of n_bound pairs)"""
    def pad(a):
        out = np.full(n_bound, sc.POISON, np.uint32)
        out[:case.n_bound] = a[:case.n_bound]
        return out
    assert case.n_dev <= case.n_bound <= n_bound
    return case._replace(keys=pad(case.keys), vals=None if case.vals is None else pad(case.vals), n_bound=n_bound)


@pytest.mark.parametrize("kind", ["pairs", "depth", "9bit"])
def test_stale_workspace(api, kind):
    """6 tiles, then 2 tiles in the very same buffers (and the other way round) without clearing anything: the histogram's row
    stride is the number of tiles the keys fill, so the second sort finds the first one's table under another stride - and
    the first one's pairs in both halves"""
    big = sc.build("count_%s_20481" % kind)
    small = widened(sc.build("count_%s_4097" % kind), big.n_bound)
    assert sc.path_of(big) == sc.path_of(small) != "small"
    for first, second in ((big, small), (small, big)):
        tmp = workspace(api, big.n_bound)
        rc, out = run(api, first, tmp)
        assert rc == 0
        check(first, out)
        rc, out = run(api, second, tmp)
        assert rc == 0
        check(second, out, tail=False)


def test_values_travel_with_keys(api):
    """values are payload - any u32, not a permutation, the all-ones word included - and the whole key travels too, the bits
    above end_bit with it"""
    case = sc.build("partition_e11_s1")
    vals = np.where(np.arange(case.vals.size) % 3 == 0, np.uint32(sc.ALL_ONES), case.vals).astype(np.uint32)
    vals[case.n_dev:] = sc.POISON
    dup = case._replace(vals=vals)
    rc, out = run(api, dup)
    assert rc == 0
    e = sc.expected(dup)
    assert int((e["vals"] == sc.ALL_ONES).sum()) >= e["n"] // 3 and int(e["keys"].max()) >= 1 << 16
    check(dup, out)
    pairs_in = np.stack([dup.keys[:e["n"]], dup.vals[:e["n"]]], 1)
    pairs_out = np.stack([out["keys"][:e["n"]], out["vals"][:e["n"]]], 1)
    assert np.array_equal(pairs_in[np.lexsort((pairs_in[:, 1], pairs_in[:, 0]))], pairs_out[np.lexsort((pairs_out[:, 1], pairs_out[:, 0]))])


@pytest.mark.parametrize("name", [c[0] for c in sc.SCAN_CASES])
def test_scan_sums(api, name):
    buf, exp = sc.scan_case(name)
    nb = buf.size - 1
    d = torch.cat([to_dev(buf), filled(64)])   # (the words behind the total must stay as they are)
    rc = api.raw("debug_scan_sums")(d.data_ptr(), nb, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    got = to_host(d)
    assert np.array_equal(got[:nb + 1].astype(np.uint64), exp), np.flatnonzero(got[:nb + 1] != exp)[:4]
    assert bool((got[nb + 1:] == sc.POISON).all())
