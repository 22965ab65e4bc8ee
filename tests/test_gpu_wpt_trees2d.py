"""wptall / iwptall / iwpdall of images with one quad tree per image (csrc/wx_wpt_trees2d.hip) against the oracle's 2-D wpt / iwpt /
iwpd called per image with that image's tree, within helpers.TOL.

Shapes, each for one way the kernel can go wrong: 8 x 8 (every node shorter than most filters: the modulo wrap goes round more than
once), 8 x 32 and 32 x 8 (row and column ranges swapped; 21 tree nodes although one side would allow more depth), 16 x 16,
64 x 64 (six levels, two items per lane), 64 x 128 Float64 / 128 x 128 Float32 (the LDS limit), 4 x 4 / 128 x 128 Float64 / 22 taps
(outside the window: the per-image fallback)."""
import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

FILTERS = ["haar", "db2", "db4", "db8", "db10"]                      # 2, 4, 8, 16 and 20 taps
TOP_LEFT, TOP_RIGHT, BOTTOM_LEFT, BOTTOM_RIGHT = 0, 1, 2, 3          # child c of node i is 4 i - 2 + c


def _levels(m, n):
    return int(min(m, n)).bit_length() - 1


def _chain(nt, depth, child):
    """the chain root -> child `child` -> ... decomposed `depth` times"""
    t = np.zeros(nt, dtype=bool)
    node = 1
    for _ in range(depth):
        t[node - 1] = True
        node = 4 * node - 2 + child
    return t


def _tree_mix(wx, m, n, rng, extra=0):
    """the batch of trees every case runs, asserted below:
    [copy, full, :dwt, chain into the top-right child, chain into the bottom-right child, random p = 0.3, 0.6, 0.9, ...]"""
    L = _levels(m, n)
    nt = wx.gettreelength(m, n)
    assert nt == (4 ** L - 1) // 3
    cols = [np.zeros(nt, dtype=bool), wx.maketree(m, n, L, "full"), wx.maketree(m, n, L, "dwt"), _chain(nt, L - 1, TOP_RIGHT),
            _chain(nt, L, BOTTOM_RIGHT)]
    seen = {c.tobytes() for c in cols}
    for i in range(3 + extra):
        p = (0.3, 0.6, 0.9)[i % 3]
        t = helpers.random_tree_2d(m, n, rng, p)
        while t.tobytes() in seen:                                    # a new tree each time (random_tree_2d always splits the root)
            t = helpers.random_tree_2d(m, n, rng, p)
        seen.add(t.tobytes())
        cols.append(t)
    trees = np.asfortranarray(np.stack(cols, axis=1))
    # the mix itself, whatever the seed gave
    assert not trees[:, 0].any() and trees[:, 1].all()
    pyramid = trees[:, 2]
    assert pyramid.sum() == L and pyramid[[(4 ** d - 1) // 3 for d in range(L)]].all()       # the chain 1, 2, 6, 22, ...
    tr, br = trees[:, 3], trees[:, 4]                                  # adjacent columns: a tree kept from the previous image shows
    assert tr[[0, 2]].all() and not tr[[1, 3, 4]].any() and br[[0, 4]].all() and not br[[1, 2, 3]].any()
    assert tr.sum() == L - 1 and br.sum() == L and br[nt - 1]          # the bottom-right chain ends in the last node of the tree
    assert len({trees[:, i].tobytes() for i in range(trees.shape[1])}) == trees.shape[1]
    assert all(wx.isvalidtree(np.zeros((m, n)), trees[:, i]) for i in range(trees.shape[1]))
    return trees


def _three(wx, m, n, rng):
    """random p = 0.9 (deep and bushy), the chain into the top-right child, the chain into the bottom-right child"""
    L = _levels(m, n)
    nt = wx.gettreelength(m, n)
    tr, br = _chain(nt, L - 1, TOP_RIGHT), _chain(nt, L, BOTTOM_RIGHT)
    rnd = helpers.random_tree_2d(m, n, rng, 0.9)
    while rnd.tobytes() in (tr.tobytes(), br.tobytes()):
        rnd = helpers.random_tree_2d(m, n, rng, 0.9)
    trees = np.asfortranarray(np.stack([rnd, tr, br], axis=1))
    assert len({trees[:, i].tobytes() for i in range(3)}) == 3
    return trees


def _per_image(fn, a, qmf, trees):
    return np.stack([fn(a[..., i], qmf, trees[:, i]) for i in range(trees.shape[1])], axis=-1)


def _check_all(wx, oracle, dtype, m, n, wname, trees, rng):
    wt = wx.wavelet(wname)                                            # by name: "db11" (22 taps) is computed, not tabulated
    tol = helpers.TOL[np.dtype(dtype)]
    B = trees.shape[1]
    x = np.asfortranarray(rng.standard_normal((m, n, B)).astype(dtype))
    # forward: every leaf at its node's own rectangle
    y = wx.wptall(x, wt, trees)
    assert y.dtype == dtype and y.shape == x.shape
    e = helpers.relerr(y, _per_image(oracle.wpt, x, wt.qmf, trees))
    print("wpt", e)
    assert e <= tol
    table = wx.wpdall(x, wt)
    e = helpers.relerr(y, wx.getbasiscoefall(table, trees))
    print("wpt vs gather", e)
    assert e <= tol
    # inverse, from coefficients that no forward transform made and as a round trip
    c = np.asfortranarray(rng.standard_normal((m, n, B)).astype(dtype))
    e = helpers.relerr(wx.iwptall(c, wt, trees), _per_image(oracle.iwpt, c, wt.qmf, trees))
    print("iwpt", e)
    assert e <= tol
    e = helpers.relerr(wx.iwptall(y, wt, trees), x)
    print("iwpt(wpt)", e)
    assert e <= tol
    # iwpd: the round trip through the table, and a table of random values
    e = helpers.relerr(wx.iwpdall(table, wt, trees), x)
    print("iwpd(wpd)", e)
    assert e <= tol
    rt = np.asfortranarray(rng.standard_normal(table.shape).astype(dtype))
    e = helpers.relerr(wx.iwpdall(rt, wt, trees), _per_image(oracle.iwpd, rt, wt.qmf, trees))
    print("iwpd", e)
    assert e <= tol


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("wname", FILTERS)
@pytest.mark.parametrize("m,n", [(8, 8), (8, 32), (32, 8), (16, 16), (64, 64)])
def test_three_families_against_the_oracle(wx, oracle, m, n, wname, dtype):
    rng = np.random.default_rng(1000 * m + 10 * n + len(wname) + ord(wname[-1]))
    trees = _tree_mix(wx, m, n, rng, extra=3)                          # 11 images: an odd batch
    assert trees.shape[1] == 11
    if (m, n) in ((8, 32), (32, 8)):
        assert trees.shape[0] == 21                                   # the shorter side decides
    _check_all(wx, oracle, dtype, m, n, wname, trees, rng)


@pytest.mark.parametrize("m,n,dtype,wname", [(64, 128, np.float64, "db4"), (64, 128, np.float64, "db10"), (128, 128, np.float32, "db4"),
                                             (128, 128, np.float32, "db10")])
def test_lds_limit(wx, oracle, m, n, dtype, wname):
    """the largest images the kernel takes: both buffers and the tree's bits fill 128.2 KiB (Float64) / 128.7 KiB (Float32) of the 160"""
    assert m * n == (8192 if dtype == np.float64 else 16384)
    rng = np.random.default_rng(m * n)
    _check_all(wx, oracle, dtype, m, n, wname, _three(wx, m, n, rng), rng)


@pytest.mark.parametrize("m,n,dtype,wname", [(4, 4, np.float64, "db2"), (128, 128, np.float64, "db4"), (16, 16, np.float32, "db11")])
def test_fallback_outside_the_window(wx, oracle, m, n, dtype, wname):
    """a side shorter than 8, more than the LDS holds, a filter of 22 taps: the single-tree path once per image inside the library"""
    rng = np.random.default_rng(m * n + len(wname))
    _check_all(wx, oracle, dtype, m, n, wname, _three(wx, m, n, rng), rng)


def test_table_with_more_slices_than_the_deepest_tree(wx, oracle):
    m = n = 16
    k, B = 5, 5
    rng = np.random.default_rng(3)
    wt = wx.wavelet(wx.WT.db4)
    nt = wx.gettreelength(m, n)
    trees = np.asfortranarray(np.stack([wx.maketree(m, n, 3, "full"), wx.maketree(m, n, 2, "dwt"), np.zeros(nt, dtype=bool),
                                        _chain(nt, 3, BOTTOM_RIGHT), _chain(nt, 1, TOP_RIGHT)], axis=1))   # depth <= 3 under a table of depth 4
    rt = np.asfortranarray(rng.standard_normal((m, n, k, B)))
    exp = _per_image(oracle.iwpd, rt, wt.qmf, trees)
    assert helpers.relerr(wx.iwpdall(rt, wt, trees), exp) <= helpers.TOL[np.dtype(np.float64)]
    with pytest.raises(wx.ArgumentError):                              # Utils.jl:120: depth 3 needs four slices
        wx.iwpdall(np.asfortranarray(rt[:, :, :3, :]), wt, trees)


def test_workgroups_take_several_images_in_turn(wx, oracle):
    """8 x 8 Float64: 64 lanes and 2 * 64 * 8 + 4 = 1028 bytes of LDS per workgroup, so the launch puts 16 workgroups (its cap)
    on each of the 256 CUs: a grid of 4096.  2 * 4096 + 5 images: workgroups 0 .. 4 take three images in turn, all others two,
    every one with another tree than the turn before.  wpt and iwpt are checked on every image, iwpd on a fixed sample with the
    first, the second and the last turns of the stride loop."""
    m = n = 8
    cus, cap = 256, 16
    lds = 2 * m * n * 8 + 4
    assert min((160 * 1024) // lds, 2048 // 64) >= cap                 # neither LDS nor lanes bind before the cap of 16 per CU
    grid = cus * cap
    B = 2 * grid + 5
    assert B > 2 * grid
    rng = np.random.default_rng(64)
    wt = wx.wavelet(wx.WT.db4)
    pool = _tree_mix(wx, m, n, rng, extra=53)                          # 61 distinct trees
    assert pool.shape[1] == 61
    b = np.arange(B)
    which = (b + b // grid) % 61                                       # the images of one workgroup (b, b + 4096, ...) differ in their trees
    assert (which[:-grid] != which[grid:]).all()
    trees = np.asfortranarray(pool[:, which])
    x = np.asfortranarray(rng.standard_normal((m, n, B)))
    tol = helpers.TOL[np.dtype(np.float64)]
    y = wx.wptall(x, wt, trees)
    assert helpers.relerr(y, _per_image(oracle.wpt, x, wt.qmf, trees)) <= tol
    assert helpers.relerr(wx.iwptall(y, wt, trees), x) <= tol
    c = np.asfortranarray(rng.standard_normal((m, n, B)))
    assert helpers.relerr(wx.iwptall(c, wt, trees), _per_image(oracle.iwpt, c, wt.qmf, trees)) <= tol
    rt = np.asfortranarray(rng.standard_normal((m, n, 4, B)))
    got = wx.iwpdall(rt, wt, trees)
    sample = np.r_[0:64, grid - 3:grid + 3, 2 * grid - 8:B]            # first, second and last turns of the stride loop
    exp = _per_image(oracle.iwpd, rt[..., sample], wt.qmf, trees[:, sample])
    assert helpers.relerr(got[..., sample], exp) <= tol


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_identical_columns_equal_the_single_tree_entry(wx, dtype):
    m = n = 64
    B = 9
    rng = np.random.default_rng(9)
    wt = wx.wavelet(wx.WT.db4)
    tree = helpers.random_tree_2d(m, n, rng, 0.7)
    assert tree[0] and not tree.all()
    trees = np.asfortranarray(np.repeat(tree[:, None], B, axis=1))
    x = np.asfortranarray(rng.standard_normal((m, n, B)).astype(dtype))
    assert (wx.wptall(x, wt, trees) == wx.wptall(x, wt, tree)).all()
    assert (wx.iwptall(x, wt, trees) == wx.iwptall(x, wt, tree)).all()
    table = wx.wpdall(x, wt)
    assert (wx.iwpdall(table, wt, trees) == wx.iwpdall(table, wt, tree)).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_host_and_device_calls_give_the_same_bits_twice(wx, dtype):
    m, n = 32, 64
    rng = np.random.default_rng(21)
    wt = wx.wavelet(wx.WT.db8)
    trees = _tree_mix(wx, m, n, rng, extra=3)
    B = trees.shape[1]
    x = np.asfortranarray(rng.standard_normal((m, n, B)).astype(dtype))
    table = wx.wpdall(x, wt)
    xd, td = wx.to_device(x), wx.to_device(table)
    for fn, host, dev in ((wx.wptall, x, xd), (wx.iwptall, x, xd), (wx.iwpdall, table, td)):
        h1 = fn(host, wt, trees)
        h2 = fn(host, wt, trees)
        d1 = wx.to_numpy(fn(dev, wt, trees))
        d2 = wx.to_numpy(fn(dev, wt, trees))
        assert h1.tobytes() == h2.tobytes() == d1.tobytes() == d2.tobytes()
        assert np.isfinite(h1).all() and np.abs(h1).max() > 0
