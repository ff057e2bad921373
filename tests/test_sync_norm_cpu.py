"""MinkowskiSyncBatchNorm.convert_sync_batchnorm without a GPU: what the conversion must keep (fuse_relu, repr,
state-dict names and shapes, parameter sharing) now that the converted layer runs on the package's kernels."""
import torch
import torch.nn as nn

import minkowskiengine_amd as ME


class _Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.a = ME.MinkowskiBatchNorm(8)
        self.a.fuse_relu = True
        self.b = ME.MinkowskiBatchNorm(4, eps=1e-3, momentum=0.05, affine=False)
        self.c = ME.MinkowskiBatchNorm(6, track_running_stats=False)


def test_conversion_copies_fuse_relu():
    net = ME.MinkowskiSyncBatchNorm.convert_sync_batchnorm(_Net())
    assert all(isinstance(m, ME.MinkowskiSyncBatchNorm) for m in (net.a, net.b, net.c))
    assert all(type(m.bn) is nn.SyncBatchNorm for m in (net.a, net.b, net.c))
    assert net.a.fuse_relu is True and net.b.fuse_relu is False and net.c.fuse_relu is False
    assert ME.MinkowskiSyncBatchNorm(8).fuse_relu is False


def test_repr_is_unchanged():
    net = ME.MinkowskiSyncBatchNorm.convert_sync_batchnorm(_Net())
    assert repr(net.a) == "MinkowskiSyncBatchNorm(8, eps=1e-05, momentum=0.1, affine=True, track_running_stats=True)"
    assert repr(net.b) == "MinkowskiSyncBatchNorm(4, eps=0.001, momentum=0.05, affine=False, track_running_stats=True)"
    assert repr(ME.MinkowskiBatchNorm(8)) == \
        "MinkowskiBatchNorm(8, eps=1e-05, momentum=0.1, affine=True, track_running_stats=True)"


def test_state_dict_names_and_shapes_survive_the_conversion():
    src = _Net()
    before = {k: tuple(v.shape) for k, v in src.state_dict().items()}
    params = dict(src.named_parameters())
    buffers = dict(src.named_buffers())
    net = ME.MinkowskiSyncBatchNorm.convert_sync_batchnorm(src)
    after = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert before and all(after.get(k) == shape for k, shape in before.items()), (before, after)
    for k, p in net.named_parameters():
        assert p is params[k], k                      # the same Parameter objects
    for k, t in net.named_buffers():
        assert t is buffers[k], k


def test_process_group_is_handed_to_the_torch_module():
    group = object()
    net = ME.MinkowskiSyncBatchNorm.convert_sync_batchnorm(_Net(), process_group=group)
    assert net.a.bn.process_group is group


def test_no_exchange_without_a_process_group():
    """torch.distributed not initialised: local statistics (torch's SyncBatchNorm does the same); CPU, float64 and
    cumulative-average layers are not for the kernels"""
    bn = ME.MinkowskiSyncBatchNorm(5).train()
    assert bn._exchange_group() is None
    assert not bn._native(torch.zeros(40, 5)) and not bn._native(torch.zeros(40, 5), min_rows=0)
    assert not ME.MinkowskiSyncBatchNorm(5, momentum=None)._native(torch.zeros(40, 5), min_rows=0)
