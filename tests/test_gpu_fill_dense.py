"""k_fill_list evaluates the live (slot quad, row) pairs of the stream layout only and writes the padding inert in a pass of its
own: the filled layout against the oracle's matrix (pattern, values, diagonal: bit for bit, as tests/test_gpu_parity.py compares
them) at the shapes where that bookkeeping can go wrong.  Small maps (n, m <= 40) throughout."""
import numpy as np
import pytest

from conftest import registration_for
from roman_amd import _abi, synth

pytestmark = pytest.mark.gpu


def check(ctx, orc, P, D1, D2, A=None):
    """Score on the device, build on the oracle: identical upper CSR.  -> the oracle's (rowptr, cols, vals, full degrees)."""
    A = None if A is None else np.ascontiguousarray(A, dtype=np.int32)
    mat, _ = orc.build_matrix(P, D1, D2, A)
    rp_o, c_o, v_o, d_o = mat.export()
    ctx.score(P, D1, D2, A)
    rp, cc, vv, dd = ctx.upper_csr()
    assert np.array_equal(rp, rp_o) and np.array_equal(cc, c_o)
    assert np.array_equal(vv, v_o) and np.array_equal(dd, d_o)
    n = len(rp_o) - 1
    rows = np.repeat(np.arange(n), np.diff(rp_o))
    deg = np.bincount(rows, minlength=n) + np.bincount(c_o, minlength=n)
    return rp_o, c_o, v_o, deg


def clipper(ctx, **kw):
    reg = registration_for("clipper", **kw); reg.set_context(ctx)
    P = reg._abi_params()
    P.mindist = 0.0
    return reg, P


def upper_counts(deg, rp, cols):
    """List length of every position (position = rank by (degree descending, row ascending)); the rows in position order."""
    n = len(deg)
    order = np.lexsort((np.arange(n), -deg)); pos = np.empty(n, dtype=np.int64); pos[order] = np.arange(n)
    rows = np.repeat(np.arange(n), np.diff(rp))
    return np.bincount(np.minimum(pos[rows], pos[cols]), minlength=n)


@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 129])
def test_last_slice_partly_empty(ctx, orc, L):
    """L = 1: one row, no entry, no slot quad at all; 63 / 64 / 65 / 129: the last slice has 63 rows, all 64, one row."""
    reg, P = clipper(ctx)
    pr = synth.make_pair(12, 12, 0, 40 + L)
    D1, D2 = reg.pack(pr.map1), reg.pack(pr.map2)
    A = orc.create_all_to_all(12, 12)[np.random.default_rng(L).permutation(144)[:L]]
    A = A[np.lexsort((A[:, 1], A[:, 0]))]
    rp, cc, _, deg = check(ctx, orc, P, D1, D2, A)
    assert len(deg) == L and (L < 63 or len(cc) > L)


def _sphere(rng, n, centre, R):
    u = rng.standard_normal((n, 3)); u /= np.linalg.norm(u, axis=1)[:, None]
    return np.vstack([centre, centre + R * u])


def test_planted_star_one_full_row_and_63_empty_ones(ctx, orc):
    """Object 0 of either map has every other object of its map at distance 10: association (0, 0) is consistent with every (i, j),
    i, j >= 1.  63 of those that are not consistent with one another: the first slice has one row with a 63-entry list (16 slot
    quads with a single live row each) and 63 rows without a list."""
    reg, P = clipper(ctx, epsilon=0.02, sigma=0.02)
    rng = np.random.default_rng(5)
    D1 = _sphere(rng, 39, np.zeros(3), 10.0); D2 = _sphere(rng, 39, np.array([3.0, -2.0, 1.0]), 10.0)
    d1 = np.linalg.norm(D1[:, None] - D1[None], axis=2); d2 = np.linalg.norm(D2[:, None] - D2[None], axis=2)
    leaves = []
    for i in range(1, 40):
        for j in range(1, 40):
            if len(leaves) < 63 and all(i == k or j == l or abs(d1[i, k] - d2[j, l]) > 0.2 for k, l in leaves):
                leaves.append((i, j))
    assert len(leaves) == 63
    A = np.array([(0, 0)] + leaves, dtype=np.int32)
    rp, cc, _, deg = check(ctx, orc, P, D1, D2, A)
    assert deg[0] == 63 and (deg[1:] == 1).all()
    assert upper_counts(deg, rp, cc).tolist() == [63] + [0] * 63


def test_clique_every_quad_tail_and_rotation_period(ctx, orc):
    """Identical maps, associations (i, i): a clique of 40.  Position p keeps 39 - p entries: every tail length (4 k + 1, + 2, + 3, + 0),
    lists of one quad (nq = 1), of five and of ten quads (multiples of FILL_ROTATE: the rotation of those rows is the identity
    for every fifth row and a pure shift for the others), and an empty last row, in one slice."""
    reg, P = clipper(ctx)
    D1 = np.random.default_rng(9).uniform(-12, 12, (40, 3))
    A = np.stack([np.arange(40), np.arange(40)], axis=1)
    rp, cc, _, deg = check(ctx, orc, P, D1, D1.copy(), A)
    cnt = upper_counts(deg, rp, cc)
    assert cnt.tolist() == list(range(39, -1, -1))
    nq = (cnt + 3) // 4
    assert {1, 5, 10} <= set(nq.tolist()) and {0, 1, 2, 3} == set((cnt % 4).tolist())


@pytest.mark.parametrize("k", [1, 5])
def test_disjoint_cliques_rows_of_4k_plus_1_entries(ctx, orc, k):
    """Map 2 holds copies of map 1's points moved by different vectors; an association joins a point with one of its copies.  Two
    associations are consistent exactly when they belong to the same copy: disjoint cliques of 4 k + 2 associations, whose first
    rows keep 4 k + 1 entries (a full last quad minus three), the following ones 4 k, 4 k - 1, ... — the cliques' rows interleave
    in the position order (equal degrees: by row), so every slice mixes all tail lengths with lists of k + 1 quads (k = 5: 6)."""
    reg, P = clipper(ctx, epsilon=0.02, sigma=0.02)
    c = 4 * k + 2
    ncl = 40 // c
    rng = np.random.default_rng(17 + k)
    D1 = rng.uniform(-10, 10, (c, 3))
    D2 = np.vstack([D1 + rng.uniform(-30, 30, 3) for _ in range(ncl)])
    A = np.array([(i, t * c + i) for i in range(c) for t in range(ncl)], dtype=np.int32)
    rp, cc, _, deg = check(ctx, orc, P, D1, D2, A)
    assert (deg == c - 1).all()
    cnt = upper_counts(deg, rp, cc)
    assert cnt.max() == 4 * k + 1 and (cnt == 4 * k + 1).sum() == ncl


def test_many_slices_several_groups_1024_threads(ctx, orc):
    """All-to-all on 40 x 40 objects: 1600 rows, 25 slices, the 1024-thread launch, several work items per problem."""
    reg, P = clipper(ctx)
    pr = synth.make_pair(40, 40, 0, 61)
    rp, cc, _, deg = check(ctx, orc, P, reg.pack(pr.map1), reg.pack(pr.map2))
    assert len(deg) == 1600 and len(cc) > 1600


def test_work_item_wider_than_one_window(ctx, orc):
    """A wide consistency test on 40 x 40 objects (rows of up to 661 entries), 64 problems in one call: a work item is then three
    consecutive slices, the first one of a problem more than 400 slot quads — more than one window of the kernel's tables (256):
    the window loop, its barriers and the slice cursor across windows.  Alone, the same problem is one slice per work item."""
    reg, P = clipper(ctx, epsilon=4.0, sigma=0.8)
    pr = synth.make_pair(40, 40, 0, 62)
    D1, D2 = reg.pack(pr.map1), reg.pack(pr.map2)
    rp, cc, _, deg = check(ctx, orc, P, D1, D2)
    cnt = upper_counts(deg, rp, cc)
    width = [(int(cnt[s:s + 64].max()) + 3) // 4 for s in range(0, len(cnt), 64)]
    assert len(width) == 25 and sum(width[:3]) > 256 + 64
    o = orc.register(P, D1, D2, reg._association_list(pr.map1, pr.map2))
    res = reg.register_and_align_batch([(pr.map1, pr.map2)] * 64)
    for b in (0, 31, 63):
        assert res.stats["nnz_upper"][b] == o["stats"].nnz_upper == len(cc) and np.array_equal(res.assoc[b], o["assoc"])
        assert res.stats["n_pass"][b] == o["stats"].n_pass


def test_filtered_entries_stay_inert(ctx, orc):
    """affinityeps at the median of the values: about half of the list entries are evaluated and dropped."""
    reg = registration_for("semanticgrav", semantics_dim=16); reg.set_context(ctx)
    pr = synth.make_pair(30, 30, 16, 78, tilt_deg=1.0)
    D1, D2 = reg.pack(pr.map1), reg.pack(pr.map2)
    P0 = reg._abi_params()
    vals = np.sort(orc.build_matrix(P0, D1, D2)[0].export()[2])
    assert vals.size > 50
    P = type(P0).from_buffer_copy(P0); P.affinityeps = float(vals[len(vals) // 2])
    rp, cc, vv, _ = check(ctx, orc, P, D1, D2)
    assert 0 < len(cc) < vals.size and (vv > P.affinityeps).all()


def test_batch_mixing_empty_problems_with_full_ones(ctx, orc):
    """Problems without a live association (an empty map; a 1 x 1 pair: one row, no entry) between full ones in one call."""
    reg = registration_for("semanticgrav", semantics_dim=16); reg.set_context(ctx)
    prs = [synth.make_pair(30, 30, 16, 300 + k, tilt_deg=1.0) for k in range(3)]
    pairs = [(prs[0].map1[:0], prs[0].map2), (prs[0].map1, prs[0].map2), (prs[1].map1[:1], prs[1].map2[:1]), (prs[2].map1, prs[2].map2)]
    res = reg.register_and_align_batch(pairs)
    assert res.status[0] & _abi.ROMAN_ST_EMPTY_MAP and res.assoc[0].shape == (0, 2)
    for b in (1, 2, 3):
        m1, m2 = pairs[b]
        o = orc.register(reg._abi_params(), reg.pack(m1), reg.pack(m2), reg._association_list(m1, m2))
        assert np.array_equal(res.assoc[b], o["assoc"]), b
        assert res.stats["n_live"][b] == o["stats"].n_live and res.stats["nnz_upper"][b] == o["stats"].nnz_upper
    assert res.stats["nnz_upper"][1] > 0 and res.stats["nnz_upper"][3] > 0
