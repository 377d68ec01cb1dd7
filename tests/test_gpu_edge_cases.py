"""Edge cases through the C ABI on the GPU: empty and ragged inputs, error conventions (status < 0 +
cs_last_error -> RuntimeError like ME), duplicates, out-of-range coordinates, tiny problems."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_error_conventions(gpu):
    from corsair_amd import _lib, backend as B

    dup = torch.tensor([[0, 1, 2, 3], [0, 1, 2, 3], [0, 0, 0, 0]], dtype=torch.int32, device=gpu)
    with pytest.raises(_lib.CorsairHipError, match="duplicate"):
        B.CoordMap.create(dup)
    far = torch.tensor([[0, 40000, 0, 0]], dtype=torch.int32, device=gpu)
    with pytest.raises(_lib.CorsairHipError, match="range"):
        B.CoordMap.create(far)
    neg = torch.tensor([[-1, 0, 0, 0]], dtype=torch.int32, device=gpu)
    with pytest.raises(_lib.CorsairHipError):
        B.CoordMap.create(neg)
    ok = B.CoordMap.create(torch.tensor([[0, 0, 0, 0], [0, 5, 5, 5]], dtype=torch.int32, device=gpu))
    km = B.KernelMap.build(ok, ok)
    x = torch.ones((2, 8), device=gpu)
    with pytest.raises(ValueError):
        B.conv_fwd(km, x, torch.ones((27, 4, 8), device=gpu))          # channel mismatch
    with pytest.raises(_lib.CorsairHipError):
        B.conv_fwd(km, torch.ones((3, 8), device=gpu), torch.ones((27, 8, 8), device=gpu))  # row mismatch
    with pytest.raises(_lib.CorsairHipError):
        B.l2_topk(torch.ones((2, 4), device=gpu), torch.ones((3, 4), device=gpu), 5)         # k > nx
    with pytest.raises(_lib.CorsairHipError):
        B.knn_feat(torch.ones((2, 16), device=gpu), [0, 2], torch.ones((4, 16), device=gpu), [0, 4], 9)
    with pytest.raises(TypeError):
        B.conv_fwd(km, x.double(), torch.ones((27, 8, 8), device=gpu))
    # the part cut reproduces KMeans(random_state=0, n_init <= 10) -- the reference's hard-coded call; the entry
    # point takes no seed (round 3: an argument that had to be 0 was a trap), more restarts than are tabulated fail
    F = torch.rand((200, 16), device=gpu)
    X = torch.rand((200, 3), device=gpu)
    anc = torch.arange(100, dtype=torch.int32, device=gpu)[None]
    with pytest.raises(_lib.CorsairHipError, match="n_init"):
        B.symcut_fit(F, X, [0, 200], anc, [2], 50, 11, 300)
    with pytest.raises(_lib.CorsairHipError):
        B.ransac_batch(X, X, [0, 200], -0.2)                              # max_corr must be positive
    # a failed call leaves the library usable
    assert B.conv_fwd(km, x, torch.ones((27, 8, 8), device=gpu)).shape == (2, 8)
    assert B.symcut_fit(F, X, [0, 200], anc, [2])[0].shape == (1, 100, 4, 3)


def test_empty_and_tiny_inputs(gpu, oracle_native):
    from corsair_amd import backend as B

    empty = B.CoordMap.create(torch.zeros((0, 4), dtype=torch.int32, device=gpu))
    assert empty.n == 0 and empty.stride(2).n == 0
    km = B.KernelMap.build(empty, empty)
    assert km.num_pairs == 0 and km.n_out == 0
    out = B.conv_fwd(km, torch.zeros((0, 32), device=gpu), torch.ones((27, 32, 32), device=gpu))
    assert out.shape == (0, 32)
    # single voxel: only the centre offset is present
    one = B.CoordMap.create(torch.tensor([[0, 3, -4, 5]], dtype=torch.int32, device=gpu))
    k1 = B.KernelMap.build(one, one)
    t = k1.table().cpu().numpy()
    assert k1.num_pairs == 1 and t[0, 13] == 0 and (np.delete(t[0], 13) == -1).all()
    w = torch.randn((27, 32, 64), device=gpu)
    x = torch.randn((1, 32), device=gpu)
    got = B.conv_fwd(k1, x, w).cpu().numpy()
    want = oracle_native.conv_fwd(t, x.cpu().numpy(), w.cpu().numpy())
    assert np.array_equal(got, want)
    # negative coordinates: floor division in the strided map
    neg = torch.tensor([[0, -1, -1, -1], [0, -2, 0, 1], [0, 1, 1, 1]], dtype=torch.int32, device=gpu)
    m = B.CoordMap.create(neg).stride(2)
    assert m.coords.cpu().numpy().tolist() == [[0, -2, -2, -2], [0, -2, 0, 0], [0, 0, 0, 0]]
    # segmented max with an absent sample, RANSAC / kNN / Chamfer with empty segments
    feats = torch.tensor([[1.0, -2.0], [3.0, -5.0], [-1.0, -1.0]], device=gpu)
    coords = torch.tensor([[0, 0, 0, 0], [0, 1, 0, 0], [2, 0, 0, 0]], dtype=torch.int32, device=gpu)
    mx = B.segmented_max(feats, coords, 3).cpu().numpy()
    assert mx[0].tolist() == [3.0, -2.0] and np.isneginf(mx[1]).all() and mx[2].tolist() == [-1.0, -1.0]
    T, inl, rmse, iters = B.ransac_batch(torch.zeros((0, 3), device=gpu), torch.zeros((0, 3), device=gpu),
                                         [0, 0, 0], 0.2, 10, 100, 0.999, 0)
    assert torch.equal(T.cpu(), torch.eye(4).repeat(2, 1, 1)) and inl.cpu().tolist() == [0, 0]
    idx = B.knn_feat(torch.ones((3, 16), device=gpu), [0, 3], torch.ones((2, 16), device=gpu), [0, 2], 5)
    assert idx.cpu().numpy()[:, :2].tolist() == [[0, 1]] * 3 and (idx.cpu().numpy()[:, 2:] == -1).all()
    cd = B.chamfer_1dir(torch.zeros((0, 3), device=gpu), [0, 0], torch.ones((2, 3), device=gpu), [0, 2],
                        [0], [0], torch.eye(4, device=gpu)[None])
    assert torch.isnan(cd).all()


def test_cad_cloud_with_fewer_voxels_than_k_is_refused_like_find_kcorr(gpu):
    """A CAD cloud with fewer than k voxels has no k-th neighbour: the reference's find_kcorr indexes with SciPy's
    out-of-range sentinel and raises IndexError (utils/eval_pose.py:66-72).  sym_pose_batch raises the same error before
    any launch (the vanilla list must never be assembled through a -1 entry), and cs_corr_assemble itself
    never turns a -1 into an address."""
    from corsair_amd import backend as B, registration as R

    rng = np.random.default_rng(0)
    F0 = torch.from_numpy(rng.standard_normal((40, 16)).astype(np.float32)).to(gpu)
    X0 = torch.from_numpy(rng.uniform(-1, 1, (40, 3)).astype(np.float32)).to(gpu)
    F1 = torch.from_numpy(rng.standard_normal((3, 16)).astype(np.float32)).to(gpu)
    X1 = torch.from_numpy(rng.uniform(-1, 1, (3, 3)).astype(np.float32)).to(gpu)
    with pytest.raises(IndexError, match="fewer than k_nn"):
        R.sym_pose_batch(F0, X0, [0, 40], F1, X1, [0, 3], [1], 5, 0.2, 0, None, 100, 500, 0.999, True, False)
    nn = B.knn_feat(F0, [0, 40], F1, [0, 3], 5)
    assert (nn.cpu().numpy()[:, 3:] == -1).all()
    desc = np.asarray([[0, 0, 0, 40, 0]], dtype=np.int64)
    src, tgt = B.corr_assemble(X0, X1, None, nn, desc, 40, 40)
    tgt = tgt.cpu().numpy().reshape(40, 5, 3)
    assert np.array_equal(tgt[:, 3], np.tile(X1[0].cpu().numpy(), (40, 1)))      # the cloud's first row, not stray memory


def test_cfg_bad_and_rows_nonfinite_flag_exactly_the_dirty_ranges(gpu):
    """cs_cfg_bad and cs_rows_nonfinite at the operator level: exactly the row ranges that hold a -1 neighbour (a short CAD
    part; over the vanilla list, a query row with a non-finite descriptor) or a non-finite element are flagged, at the
    first and last entry of a range, next to an empty range, and a finite 1e30 is not."""
    from corsair_amd import backend as B

    rng = np.random.default_rng(9)
    first = [0, 3, 3, 10, 300, 301, 700]
    nn = rng.integers(0, 50, (700, 5)).astype(np.int32)
    nn[2, 4] = -1          # last entry of range 0
    nn[10, 0] = -1         # first entry of range 3 (not the last of range 2)
    nn[699, 2] = -1        # last row of the last range
    first_t = torch.tensor(first, dtype=torch.int64, device=gpu)
    bad = B.cfg_bad(torch.from_numpy(nn).to(gpu), first_t, 6).cpu().numpy()
    assert bad.tolist() == [int((nn[a:b] < 0).any()) for a, b in zip(first[:-1], first[1:])] == [1, 0, 0, 1, 0, 1]
    x = rng.standard_normal((700, 16)).astype(np.float32)
    x[9, 15] = np.nan
    x[300, 0] = -np.inf
    x[500, 7] = 1e30       # finite
    bad = B.rows_nonfinite(torch.from_numpy(x).to(gpu), first_t, 6).cpu().numpy()
    assert bad.tolist() == [0, 0, 1, 0, 1, 0]


def test_ragged_batch_forward_row_order(gpu):
    """Batch of clouds with very different sizes: per-sample row segments stay in input order."""
    from corsair_amd import engine, synth
    from tests.helpers import make_batch

    coords, feats, _, offsets = make_batch([60, 61, 62], n_points=800)
    coords2, feats2, _, _ = make_batch([63], n_points=9000)
    coords2[:, 0] = 3
    allc = np.concatenate([coords, coords2])
    sd, emb = synth.make_state_dicts(31)
    eng = engine.ResUNetEngine(sd, emb, device=gpu)
    out, feat, maps = eng.forward(torch.from_numpy(allc).to(gpu),
                                  torch.ones((len(allc), 1), device=gpu))
    assert np.array_equal(maps.c1.coords.cpu().numpy(), allc)
    g = eng.embed(feat, maps, 4)
    # each sample's result is independent of its batch mates: rerun the big cloud alone
    solo = coords2.copy()
    solo[:, 0] = 0
    out1, feat1, maps1 = eng.forward(torch.from_numpy(solo).to(gpu), torch.ones((len(solo), 1), device=gpu))
    g1 = eng.embed(feat1, maps1, 1)
    assert torch.equal(out[len(coords):], out1) and torch.equal(g[3], g1[0])


def test_handles_dropped_on_another_thread_do_not_enter_its_cache(gpu):
    """coordinate / kernel maps are freed from Python __del__, which runs on whichever
    thread drops the last reference.  Scratch is cached per thread in stream order, so a block freed
    by a foreign thread must not be recycled there (its owner's stream may still read it): the pool
    releases it with hipFree instead.  Maps are built (and used) on a worker thread with its own
    stream, dropped on the main thread; the results stay right and the pool reports the foreign frees."""
    import ctypes
    import threading

    from corsair_amd import _lib, backend as B, engine
    from tests.helpers import make_batch

    lib = _lib.load()
    stats = (ctypes.c_uint64 * 3)()
    lib.cs_pool_stats(stats)
    foreign0 = int(stats[1])
    coords, feats, _, _ = make_batch([0, 1], n_points=3000)
    grid = torch.from_numpy(coords).to(gpu)
    x = torch.from_numpy(feats).to(gpu)
    w = torch.full((27, 1, 32), 0.25, device=gpu)
    box = {}

    def worker():
        torch.cuda.set_device(gpu)
        st = torch.cuda.Stream(device=gpu)
        with torch.cuda.stream(st):
            m = engine.BatchMaps(grid)
            box["y"] = B.conv_fwd(m.s1, x, w)
            box["maps"] = m            # the last reference leaves this thread alive
            st.synchronize()

    t = threading.Thread(target=worker)
    t.start()
    t.join()
    want = B.conv_fwd(engine.BatchMaps(grid).s1, x, w)
    assert torch.equal(box["y"], want)
    live_before = None
    lib.cs_pool_stats(stats)
    live_before = int(stats[0])
    del box["maps"]                    # __del__ -> cs_kernelmap_free / cs_coordmap_free on THIS thread
    import gc

    gc.collect()
    lib.cs_pool_stats(stats)
    assert int(stats[1]) > foreign0, "blocks freed by a foreign thread were not detected"
    assert int(stats[0]) < live_before
    # this thread's cache did not receive them: a fresh build here still computes the right thing
    again = B.conv_fwd(engine.BatchMaps(grid).s1, x, w)
    assert torch.equal(again, want)
