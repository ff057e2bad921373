"""GPU tests of direct max pooling (csrc/direct_pool.hip through both host layers): bit-equality with the reference's
fixtures, the cases the reference's CPU kernel gets wrong against a numpy restatement of its GPU rule, errors,
gradcheck, determinism, host equality and the per-voxel max recipe for a TensorField."""
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "direct_pool_*.npz")))
IDS = [os.path.basename(p)[:-4] for p in FIXTURES]


def _me():
    import minkowskiengine_amd as ME
    return ME


def _C():
    from minkowskiengine_amd import host
    return host.backend()


def _rule(in_map, out_map, feat, out_nrows):
    """numpy restatement of the GPU rule: `max < cur` from the row's first entry in map order; empty rows 0 / marker"""
    im, om = np.asarray(in_map, np.int64), np.asarray(out_map, np.int64)
    c = feat.shape[1]
    out = np.zeros((out_nrows, c), feat.dtype)
    idx = np.full((out_nrows, c), np.iinfo(np.asarray(in_map).dtype).max, np.asarray(in_map).dtype)
    started = np.zeros(out_nrows, bool)
    for e in range(len(im)):
        o, r = om[e], im[e]
        for ch in range(c):
            if not started[o] or out[o, ch] < feat[r, ch]:
                out[o, ch] = feat[r, ch]
                idx[o, ch] = r * c + ch
        started[o] = True
    return out, idx


def _rule_backward(grad_out, idx, in_nrows):
    c = grad_out.shape[1]
    g = np.zeros((in_nrows, c), np.float64)
    valid = (idx >= 0) & (idx < in_nrows * c)
    np.add.at(g.reshape(-1), idx[valid].astype(np.int64), grad_out[valid].astype(np.float64))
    return g


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_reference_fixtures_bit_equal(path, host_layer, device):
    z = np.load(path)
    C = _C()
    im, om = torch.from_numpy(z["in_map"]).to(device), torch.from_numpy(z["out_map"]).to(device)
    f = torch.from_numpy(z["in_feat"]).to(device)
    out, idx = C.direct_max_pool_fw(im, om, f, int(z["out_nrows"]), bool(z["is_sorted"]))
    assert idx.dtype == im.dtype and out.dtype == f.dtype
    assert np.array_equal(out.cpu().numpy(), z["out_feat"])
    assert np.array_equal(idx.cpu().numpy(), z["max_index"])
    g = C.direct_max_pool_bw(torch.from_numpy(z["grad_out"]).to(device), idx, f.shape[0])
    assert np.array_equal(g.cpu().numpy(), z["grad_in"])
    if not bool(z["is_sorted"]):       # the sort is this library's: a sorted copy with the flag gives the same
        order = torch.argsort(om, stable=True)
        out2, idx2 = C.direct_max_pool_fw(im[order], om[order], f, int(z["out_nrows"]), True)
        assert torch.equal(out, out2) and torch.equal(idx, idx2)


def test_reference_fixtures_bf16(host_layer, device):
    skipped = 0
    for path in FIXTURES:
        z = np.load(path)
        f = torch.from_numpy(z["in_feat"]).to(torch.bfloat16)
        fr = f.float().numpy()
        im, om = z["in_map"].astype(np.int64), z["out_map"].astype(np.int64)
        tie = any(len(np.unique(fr[im[om == o], ch])) != int((om == o).sum())
                  for o in range(int(z["out_nrows"])) for ch in range(fr.shape[1]))
        if tie:
            skipped += 1
            continue
        out, idx = _C().direct_max_pool_fw(torch.from_numpy(z["in_map"]).to(device),
                                           torch.from_numpy(z["out_map"]).to(device), f.to(device),
                                           int(z["out_nrows"]), bool(z["is_sorted"]))
        assert out.dtype == torch.bfloat16
        assert np.array_equal(idx.cpu().numpy(), z["max_index"])
        want = f.reshape(-1)[torch.from_numpy(z["max_index"].astype(np.int64))]
        assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))
    assert skipped <= 1


@pytest.mark.parametrize("itype", [torch.int32, torch.int64])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16])
def test_negative_empty_ties_shared(itype, dtype, host_layer, device):
    """all-negative rows, empty output rows, ties (first entry wins) and input rows under several outputs"""
    C = _C()
    g = torch.Generator().manual_seed(3)
    n_in, n_out, c, nmap = 40, 12, 8, 90
    f = -(torch.randint(1, 6, (n_in, c), generator=g).float())           # negative, many ties
    f[::7] = torch.randint(-3, 4, (len(f[::7]), c), generator=g).float()
    im = torch.randint(0, n_in, (nmap,), generator=g)
    om = torch.randint(0, n_out, (nmap,), generator=g)
    om[om == 4] = 5
    om[om == 9] = 0                                                      # rows 4 and 9 stay empty
    fd = f.to(dtype)
    out, idx = C.direct_max_pool_fw(im.to(itype).to(device), om.to(itype).to(device), fd.to(device), n_out, False)
    want, widx = _rule(im.to(itype).numpy(), om.numpy(), f.numpy(), n_out)
    assert np.array_equal(out.float().cpu().numpy(), want)
    assert np.array_equal(idx.cpu().numpy(), widx)
    marker = torch.iinfo(itype).max
    assert bool((idx[4] == marker).all()) and bool((idx[9] == marker).all())
    assert bool((out[4] == 0).all()) and bool((out[9] == 0).all())
    go = torch.randn(n_out, c, generator=g).to(dtype)
    g1 = C.direct_max_pool_bw(go.to(device), idx, n_in)
    g2 = C.direct_max_pool_bw(go.to(device), idx, n_in)
    assert torch.equal(g1, g2)                                           # sums of several winners: run to run
    wg = _rule_backward(go.float().numpy(), widx, n_in)
    tol = 1e-12 if dtype == torch.float64 else (1e-5 if dtype == torch.float32 else 5e-2)
    np.testing.assert_allclose(g1.double().cpu().numpy(), wg, atol=tol, rtol=tol)
    assert bool((np.bincount(widx[widx < marker].astype(np.int64)) > 1).any())   # the case does hold shared winners


_WIDTH_CASES = [(torch.float32, 8), (torch.float32, 6), (torch.float32, 7), (torch.bfloat16, 16), (torch.bfloat16, 12),
                (torch.bfloat16, 7), (torch.float64, 4), (torch.float64, 3)]


@pytest.mark.parametrize("itype", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("dtype,c", _WIDTH_CASES, ids=[f"{str(d)[6:]}-c{c}" for d, c in _WIDTH_CASES])
def test_piece_widths_and_unaligned_views(dtype, c, itype, device):
    """The piece of k_direct_max follows c and the addresses of in_feat, out_feat and max_index (16 bytes, 8 bytes, one
    channel: fp32 c = 8 / 6 / 7, bf16 16 / 12 / 7, float64 4 / 3); a maximum and its index do not depend on the width.
    in_feat and out_feat go 8 bytes and one element into their storage, one at a time and together; then, on allocator
    addresses, max_index alone goes half a wide mask piece (and one element) into its storage, so that only the mask
    forbids the wide piece.  Outputs and masks bit-equal to the call on allocator addresses, which is the backend's."""
    from helpers import placed
    from minkowskiengine_amd import _lib, backend
    lib = _lib.load()
    fn = getattr(lib, "me_direct_max_pool_" + {torch.float32: "f32", torch.bfloat16: "bf16", torch.float64: "f64"}[dtype])
    rng = np.random.default_rng(c)
    n_in, n_out = 700, 500
    om = rng.permutation(np.repeat(np.arange(n_out), rng.integers(1, 5, n_out)))     # 1 to 4 inputs per output row
    nmap = len(om)
    im = torch.from_numpy(rng.integers(0, n_in, nmap)).to(itype).to(device)
    om = torch.from_numpy(om).to(itype).to(device)
    x = torch.from_numpy(rng.integers(-8, 9, (n_in, c)) / 4.0).to(dtype).to(device)   # exact in bf16, with ties
    ws = torch.empty(lib.me_direct_max_pool_workspace_bytes(nmap, n_out), dtype=torch.uint8, device=device)
    stream = torch.cuda.current_stream(device).cuda_stream
    bits = lambda t: t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])  # noqa: E731

    def run(hx="alloc", hy="alloc", mask_pad=0):
        px, y = placed(x, hx), placed(torch.zeros(n_out, c, dtype=dtype, device=device), hy)
        buf = torch.zeros(mask_pad + n_out * c, dtype=itype, device=device)
        mask = buf[mask_pad:].view(n_out, c)
        assert buf.data_ptr() % 64 == 0 and mask.data_ptr() == buf.data_ptr() + mask_pad * buf.element_size()
        with torch.cuda.device(device):
            _lib.check(fn(px.data_ptr(), c, im.data_ptr(), om.data_ptr(), im.element_size(), nmap, n_in, n_out, 0,
                          y.data_ptr(), mask.data_ptr(), ws.data_ptr(), ws.numel(), stream))
        return bits(y), mask.clone()

    want = run()
    mine = backend.direct_max_pool_fw(im, om, x, n_out, False)
    assert torch.equal(want[0], bits(mine[0])) and torch.equal(want[1], mine[1])
    wide = 16 // x.element_size()
    pads = sorted({wide // 2, 1} if c % wide == 0 else {1})  # half a wide mask piece: aligned for the 8-byte piece only
    cases = [dict(hx=o) for o in ("8", "1")] + [dict(hy=o) for o in ("8", "1")] + [dict(hx=o, hy=o) for o in ("8", "1")] + \
        [dict(mask_pad=p) for p in pads]
    for how in cases:
        got = run(**how)
        assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1]), how


def test_tie_first_entry_wins(host_layer, device):
    C = _C()
    f = torch.tensor([[1.0], [1.0], [1.0], [0.5]], device=device)
    im = torch.tensor([2, 0, 1, 3], device=device)
    om = torch.tensor([0, 0, 0, 0], device=device)
    out, idx = C.direct_max_pool_fw(im, om, f, 1, False)
    assert idx.tolist() == [[2]] and out.tolist() == [[1.0]]
    out, idx = C.direct_max_pool_fw(im.flip(0).contiguous(), om, f, 1, True)
    assert idx.tolist() == [[1]]


def test_empty_map_and_errors(host_layer, device):
    C = _C()
    f = torch.rand(5, 3, device=device)
    e = torch.zeros(0, dtype=torch.long, device=device)
    out, idx = C.direct_max_pool_fw(e, e, f, 4, False)
    assert out.shape == (4, 3) and bool((out == 0).all()) and bool((idx == torch.iinfo(torch.int64).max).all())
    g = C.direct_max_pool_bw(torch.rand(4, 3, device=device), idx, 5)
    assert g.shape == (5, 3) and bool((g == 0).all())
    im = torch.tensor([0, 1, 2, 3], device=device)
    with pytest.raises(RuntimeError):           # three distinct outputs {0, 5, 7}, out_nrows 2
        C.direct_max_pool_fw(im, torch.tensor([0, 5, 7, 0], device=device), f, 2, False)
    with pytest.raises(RuntimeError):
        C.direct_max_pool_fw(torch.tensor([0, 1, 2, 5], device=device), torch.tensor([0, 1, 1, 0], device=device), f, 2)
    with pytest.raises(RuntimeError):
        C.direct_max_pool_fw(torch.tensor([0, -1, 2, 3], device=device), torch.tensor([0, 1, 1, 0], device=device), f, 2)
    with pytest.raises(RuntimeError):
        C.direct_max_pool_fw(im, torch.tensor([0, -1, 1, 0], device=device), f, 2, False)
    with pytest.raises(RuntimeError):           # dtype / length mismatch
        C.direct_max_pool_fw(im.int(), torch.tensor([0, 1, 1, 0], device=device), f, 2, False)
    with pytest.raises(RuntimeError):
        C.direct_max_pool_fw(im[:3], torch.tensor([0, 1, 1, 0], device=device), f, 2, False)
    with pytest.raises(RuntimeError):           # CPU tensors
        C.direct_max_pool_fw(im.cpu(), torch.tensor([0, 1, 1, 0]), f.cpu(), 2, False)
    with pytest.raises(RuntimeError):
        C.direct_max_pool_fw(im.cpu(), torch.tensor([0, 1, 1, 0]), f, 2, False)


def test_maps_are_not_modified(host_layer, device):
    C = _C()
    g = torch.Generator().manual_seed(1)
    im = torch.randperm(50, generator=g).to(device)
    om = torch.randint(0, 9, (50,), generator=g).to(device)
    im0, om0 = im.clone(), om.clone()
    C.direct_max_pool_fw(im, om, torch.rand(50, 4, device=device), 9, False)
    assert torch.equal(im, im0) and torch.equal(om, om0)


def test_gradcheck_float64(host_layer, device):
    ME = _me()
    g = torch.Generator().manual_seed(5)
    n_in, n_out, c = 30, 7, 3
    f = torch.stack([torch.randperm(n_in, generator=g).double() / n_in - 0.5 for _ in range(c)], 1).to(device)
    f.requires_grad_(True)
    im = torch.cat([torch.randperm(n_in, generator=g), torch.randint(0, n_in, (12,), generator=g)]).to(device)
    om = torch.randint(0, n_out - 1, (len(im),), generator=g).to(device)        # the last output row stays empty
    fn = lambda x: ME.MinkowskiDirectMaxPoolingFunction.apply(im, om, x, n_out)   # noqa: E731
    assert torch.autograd.gradcheck(fn, (f,), eps=1e-6, atol=1e-6, rtol=1e-4)


def test_hosts_bit_equal_and_three_argument_backward(device):
    from minkowskiengine_amd import backend, host
    native = host.native_module()
    assert native is not None, host.native_error()
    g = torch.Generator().manual_seed(9)
    for dtype, c in ((torch.float32, 20), (torch.bfloat16, 24), (torch.float64, 5), (torch.float32, 96)):
        n_in, n_out, nmap = 3000, 700, 5000
        f = torch.randn(n_in, c, generator=g).to(dtype).to(device)
        im = torch.randint(0, n_in, (nmap,), generator=g).to(device)
        om = torch.randint(0, n_out, (nmap,), generator=g).to(device)
        go = torch.randn(n_out, c, generator=g).to(dtype).to(device)
        o1, i1 = backend.direct_max_pool_fw(im, om, f, n_out, False)
        o2, i2 = native.direct_max_pool_fw(im, om, f, n_out, False)
        assert torch.equal(o1, o2) and torch.equal(i1, i2)
        g1 = backend.direct_max_pool_bw(go, i1, n_in)                   # exactly three arguments, as the reference calls
        g2 = native.direct_max_pool_bw(go, i2, n_in)
        assert torch.equal(g1, g2)
        want, widx = _rule(im.cpu().numpy(), om.cpu().numpy(), f.float().cpu().numpy().astype(np.float64), n_out)
        assert np.array_equal(i1.cpu().numpy(), widx)
        assert np.array_equal(o1.double().cpu().numpy(), want)


def test_field_max_recipe(host_layer, device):
    """field -> field_to_sparse_insert_and_map -> the function = numpy per-voxel max; sparse(MAX_POOL) still raises"""
    ME = _me()
    z = np.load(os.path.join(ROOT, "tests", "golden", "field_3d_s1.npz"))
    c = torch.from_numpy(z["field_coords"]).to(device)
    f = torch.from_numpy(z["field_feats"]).to(device).requires_grad_(True)
    tf = ME.TensorField(f, coordinates=c, quantization_mode=ME.SparseTensorQuantizationMode.MAX_POOL)
    with pytest.raises(NotImplementedError):
        tf.sparse()
    mgr = tf.coordinate_manager
    key, (_, inv) = mgr.field_to_sparse_insert_and_map(tf.coordinate_field_map_key, [1, 1, 1])
    n_vox = mgr.size(key)
    F = ME.MinkowskiDirectMaxPoolingFunction.apply(torch.arange(len(tf), device=device), inv, tf.F, n_vox)
    s = ME.SparseTensor(F, coordinate_map_key=key, coordinate_manager=mgr)
    assert s.F.shape == (n_vox, f.shape[1])
    invn, fn = inv.cpu().numpy(), z["field_feats"]
    want = np.stack([fn[invn == v].max(0) for v in range(n_vox)])
    assert np.array_equal(s.F.detach().cpu().numpy(), want)
    s.F.sum().backward()
    hit = np.zeros_like(fn)
    for v in range(n_vox):
        rows = np.nonzero(invn == v)[0]
        hit[rows[fn[rows].argmax(0)], np.arange(fn.shape[1])] += 1
    assert np.array_equal(f.grad.cpu().numpy(), hit)
