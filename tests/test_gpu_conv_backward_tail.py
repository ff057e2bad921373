"""Backward pass of a split-fp32 convolution in two launches — the weight gradient's partial images, then the input
gradient whose trailing workgroups reduce them (k_conv_tile_f32x3_ws<..., TAIL>, wgrad_reduce.hpp) — against the three
launches it replaces (input gradient, weight gradient, k_wgrad_reduce): both gradients BIT-identical, and within the
fp32 bar of the float64 oracle.  me_debug_set_dgrad_reduce_tail picks the order: 1 = three launches, 2 = two launches
wherever the kernels exist, 0 = the shipped policy.  Which order ran is read off the launch timer's labels: the
two-launch order records "conv_wgrad" BEFORE "conv_dgrad", the three-launch order after it."""
import numpy as np
import pytest
import torch

from helpers import assert_close, make_cloud

pytestmark = pytest.mark.gpu

THREE, TWO, POLICY = 1, 2, 0


def _lib():
    from minkowskiengine_amd import _lib
    return _lib.load()


def _labels(step):
    """the launch timer's labels of one call of step(), in launch order"""
    import minkowskiengine_amd as ME
    import minkowskiengine_amd.backend as MEB
    from minkowskiengine_amd import host
    nm = host.native_module() if ME.is_native() else None
    timer = MEB.KernelTimer()
    MEB.KERNEL_TIMER = timer
    if nm is not None:
        nm.timing_records(True)
        nm.timing_enable(True)
    try:
        step()
        torch.cuda.synchronize()
        names = [r[0] for r in nm.timing_records(True)] if nm is not None else list(timer.events)
    finally:
        MEB.KERNEL_TIMER = None
        if nm is not None:
            nm.timing_enable(False)
    return [n for n in names if n in ("conv_dgrad", "conv_wgrad")]


class Layer:
    """one MinkowskiConvolution (k = 3, D = 3) on fixed inputs; run(mode) -> (grad_in | None, grad_w, labels)"""

    def __init__(self, device, coords, cin, cout, seed=0, dtype=torch.float32, x_grad=True):
        g = torch.Generator().manual_seed(seed)
        self.device, self.coords, self.cin, self.cout, self.dtype, self.x_grad = device, coords, cin, cout, dtype, x_grad
        self.feats = (torch.rand(coords.shape[0], cin, generator=g) - 0.4)
        self.w = torch.rand(27, cin, cout, generator=g) - 0.5
        self.gy = torch.rand(coords.shape[0], cout, generator=g) - 0.5

    def run(self, mode, passes=1):
        import minkowskiengine_amd as ME
        lib = _lib()
        ME.clear_global_coordinate_manager()
        conv = ME.MinkowskiConvolution(self.cin, self.cout, kernel_size=3, dimension=3).to(self.device)
        with torch.no_grad():
            conv.kernel.copy_(self.w)
        x = ME.SparseTensor(self.feats.to(self.dtype).to(self.device), self.coords.to(self.device),
                            requires_grad=self.x_grad)
        gy = self.gy.to(self.dtype).to(self.device)

        def step():
            conv(x).F.backward(gy)

        lib.me_debug_set_dgrad_reduce_tail(mode)
        try:
            labels = _labels(step)
            for _ in range(passes - 1):
                step()
            torch.cuda.synchronize()
        finally:
            lib.me_debug_set_dgrad_reduce_tail(POLICY)
            ME.clear_global_coordinate_manager()
        return (x.F.grad.clone() if self.x_grad else None), conv.kernel.grad.clone(), labels

    def oracle(self):
        from oracle import me_oracle as O
        co = self.coords.numpy()
        _, km = O.kernel_map(co, co, O.make_region(3, 3))
        gi, gw = O.conv_backward(self.feats.numpy().astype(np.float64), self.gy.numpy().astype(np.float64),
                                 self.w.numpy().astype(np.float64), km)
        return gi, gw, km


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check_pair(layer, want_two=True):
    gi3, gw3, l3 = layer.run(THREE)
    gi2, gw2, l2 = layer.run(TWO)
    assert l3 == ["conv_dgrad", "conv_wgrad"], l3
    assert l2 == (["conv_wgrad", "conv_dgrad"] if want_two else ["conv_dgrad", "conv_wgrad"]), l2
    assert _same_bits(gw2, gw3), "grad_w differs between the two-launch and the three-launch order"
    assert _same_bits(gi2, gi3), "the input gradient differs between the two-launch and the three-launch order"
    return gi2, gw2


def plane_cloud(n_side):
    """a one-voxel-thick plane z = 3: the 18 offsets with dz != 0 have no pairs"""
    ij = torch.stack(torch.meshgrid(torch.arange(n_side), torch.arange(n_side), indexing="ij"), -1).reshape(-1, 2)
    c = torch.cat([torch.zeros(len(ij), 1, dtype=torch.long), ij, torch.full((len(ij), 1), 3)], 1)
    return c[torch.randperm(len(c), generator=torch.Generator().manual_seed(3))].int().contiguous()


def isolated_cloud(n):
    """voxels on the even lattice: no voxel has a neighbour, every pair belongs to the centre offset"""
    c = make_cloud(n, 20, 3, seed=5)
    c[:, 1:] *= 2
    return c


# 64 -> 128: the input-gradient slab is 64 columns, 512 threads, two groups per tail workgroup;
# 128 -> 128: 128 columns, 768 threads, three groups; 128 -> 64: the same slab over one-block images (nb = 1).
# 300 voxels in 8^3: one to three tiles; 10 voxels: less than a tile
@pytest.mark.parametrize("cin,cout,n", [(64, 128, 300), (128, 128, 300), (64, 128, 10), (128, 128, 10), (128, 64, 300)])
def test_two_launch_order_is_bit_identical_and_matches_the_oracle(device, cin, cout, n):
    layer = Layer(device, make_cloud(n, 8, 3, seed=n + cin), cin, cout)
    gi, gw = _check_pair(layer)
    ogi, ogw, _ = layer.oracle()
    assert_close(gi, ogi, what="grad_in")
    assert_close(gw, ogw, what="grad_w")


def test_offsets_without_pairs_get_exact_zeros(device):
    layer = Layer(device, plane_cloud(12), 64, 128)
    gi, gw = _check_pair(layer)
    ogi, ogw, km = layer.oracle()
    empty = [k for k in range(27) if not np.any(ogw[k])]
    assert len(empty) == 18
    for k in empty:
        assert torch.count_nonzero(gw[k]).item() == 0 and not torch.signbit(gw[k]).any().item()
    assert_close(gi, ogi, what="grad_in")
    assert_close(gw, ogw, what="grad_w")


def test_more_slots_than_one_round_of_eight_per_phase(device):
    """2880 isolated voxels: 45 ranges of 64 pairs, all of the centre offset — 45 slots, so each of the four phases
    takes one full round of eight loads and a remainder of three or four"""
    layer = Layer(device, isolated_cloud(2880), 64, 128)
    assert layer.coords.shape[0] == 2880
    gi, gw = _check_pair(layer)
    ogi, ogw, _ = layer.oracle()
    assert np.count_nonzero([np.any(ogw[k]) for k in range(27)]) == 1
    assert_close(gi, ogi, what="grad_in")
    assert_close(gw, ogw, what="grad_w")


def test_non_finite_values_give_the_same_result_class(device):
    layer = Layer(device, make_cloud(300, 8, 3, seed=9), 64, 128)
    layer.feats[5, 3] = float("inf")
    layer.feats[17, 60] = float("nan")
    layer.gy[7, 2] = float("nan")
    layer.gy[40, 100] = float("-inf")
    gi3, gw3, _ = layer.run(THREE)
    gi2, gw2, l2 = layer.run(TWO)
    assert l2 == ["conv_wgrad", "conv_dgrad"]
    for a, b in ((gi2, gi3), (gw2, gw3)):
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.isinf(a), torch.isinf(b))
        assert torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
    assert torch.isnan(gw2).any() and torch.isnan(gi2).any()


def test_input_without_requires_grad_keeps_the_weight_gradient_launches(device):
    layer = Layer(device, make_cloud(300, 8, 3, seed=2), 64, 128, x_grad=False)
    _, gw3, l3 = layer.run(THREE)
    _, gw2, l2 = layer.run(TWO)
    assert l3 == ["conv_wgrad"] and l2 == ["conv_wgrad"]
    assert _same_bits(gw2, gw3)
    assert_close(gw2, layer.oracle()[1], what="grad_w")


@pytest.mark.parametrize("cin,cout,dtype", [(64, 128, torch.bfloat16), (96, 128, torch.float32)])
def test_other_kernels_keep_three_launches(device, cin, cout, dtype):
    """bf16 features, and an input gradient of 96 columns (the ping-pong kernel, no wave-specialised one): the old order
    whatever the switch says"""
    layer = Layer(device, make_cloud(300, 8, 3, seed=4), cin, cout, dtype=dtype)
    gi3, gw3, l3 = layer.run(THREE)
    gi2, gw2, l2 = layer.run(TWO)
    assert l3 == l2 == ["conv_dgrad", "conv_wgrad"]
    assert torch.equal(gw2, gw3) and torch.equal(gi2, gi3)
    if dtype == torch.float32:
        assert _lib().me_conv_dgrad_reduce_tail_supported(cin, cout, 27, 5000) == 0


def test_policy_takes_the_tail_only_while_it_is_short(device):
    """the shipped policy: the headline layer (64 -> 128: 432 tail workgroups) and layers up to 128 -> 256 (1152) run in
    two launches; 256 input channels (two slab rows of tiles; 256 -> 256: 2304 tail workgroups of one per CU) keep the
    reduce launch"""
    lib = _lib()
    for cin, cout, want in ((64, 128, 1), (128, 128, 1), (128, 256, 1), (256, 128, 0), (256, 256, 0),
                            (96, 128, 0),      # 96-column input gradient: no wave-specialised kernel
                            (16, 32, 0)):      # not the split weight gradient
        assert lib.me_conv_dgrad_reduce_tail_supported(cin, cout, 27, 834914) == want, (cin, cout)
    layer = Layer(device, make_cloud(300, 8, 3, seed=6), 64, 128)
    assert layer.run(POLICY)[2] == ["conv_wgrad", "conv_dgrad"]


def test_python_host_takes_the_same_order_with_the_same_bits(device):
    import minkowskiengine_amd as ME
    layer = Layer(device, make_cloud(300, 8, 3, seed=11), 64, 128)
    prev = ME.get_host()
    try:
        ME.set_host("python")
        gi_p, gw_p = _check_pair(layer)
    finally:
        ME.set_host(prev)
        ME.clear_global_coordinate_manager()
    gi, gw, _ = layer.run(TWO)
    assert _same_bits(gw_p, gw) and _same_bits(gi_p, gi)


def test_second_backward_pass_accumulates(device):
    layer = Layer(device, make_cloud(300, 8, 3, seed=7), 64, 128)
    gi3, gw3, _ = layer.run(THREE, passes=2)
    gi2, gw2, _ = layer.run(TWO, passes=2)
    assert _same_bits(gw2, gw3) and _same_bits(gi2, gi3)
    gi1, gw1, _ = layer.run(TWO, passes=1)
    assert torch.equal(gw2, gw1 + gw1) and torch.equal(gi2, gi1 + gi1)


def test_captured_graph_replays_the_two_launch_step(device):
    """forward + backward of one layer captured once (a single chain on the capture stream: no side stream, no events)
    and replayed on new input values"""
    import minkowskiengine_amd as ME
    lib = _lib()
    layer = Layer(device, make_cloud(300, 8, 3, seed=8), 64, 128)
    gi3, gw3, _ = layer.run(THREE)
    ME.clear_global_coordinate_manager()
    conv = ME.MinkowskiConvolution(64, 128, kernel_size=3, dimension=3).to(device)
    with torch.no_grad():
        conv.kernel.copy_(layer.w)
    feats = torch.zeros_like(layer.feats).to(device)
    x = ME.SparseTensor(feats, layer.coords.to(device), requires_grad=True)
    gy = layer.gy.to(device)

    def step():
        x.F.grad = None
        conv.kernel.grad = None
        conv(x).F.backward(gy)

    graph = None
    lib.me_debug_set_dgrad_reduce_tail(TWO)
    try:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                step()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step()
        with torch.no_grad():
            x.F.copy_(layer.feats.to(device))     # the values the three-launch reference saw
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(conv.kernel.grad, gw3) and _same_bits(x.F.grad, gi3)
    finally:
        lib.me_debug_set_dgrad_reduce_tail(POLICY)
        del graph
        ME.clear_global_coordinate_manager()
