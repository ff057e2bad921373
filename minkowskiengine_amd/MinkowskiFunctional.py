"""Functional twins of torch.nn.functional on sparse tensors and tensor fields (the reference's MinkowskiFunctional.py):
the torch function runs on the feature matrix `.F`.  Activations and the other feature-to-feature functions return a
tensor of the input's kind on the input's coordinates (a TensorField stays a TensorField); losses take a torch target
and return what torch returns.  No kernels of their own."""
import torch.nn.functional as F

from .layers import _rewrap

_FEATURE_FUNCTIONS = (
    "threshold", "relu", "hardtanh", "hardswish", "relu6", "elu", "selu", "celu", "leaky_relu", "prelu", "rrelu", "glu",
    "gelu", "logsigmoid", "hardshrink", "tanhshrink", "softsign", "softplus", "softmin", "softmax", "softshrink",
    "gumbel_softmax", "log_softmax", "tanh", "sigmoid", "hardsigmoid", "silu", "batch_norm", "normalize", "linear",
    "dropout", "alpha_dropout")
_LOSSES = (
    "binary_cross_entropy", "binary_cross_entropy_with_logits", "poisson_nll_loss", "cross_entropy",
    "hinge_embedding_loss", "kl_div", "l1_loss", "mse_loss", "multilabel_margin_loss", "multilabel_soft_margin_loss",
    "multi_margin_loss", "nll_loss", "smooth_l1_loss", "soft_margin_loss")


def _feature_function(name):
    fn = getattr(F, name)

    def wrapped(input, *args, **kwargs):
        return _rewrap(input, fn(input.F, *args, **kwargs))
    wrapped.__name__ = wrapped.__qualname__ = name
    wrapped.__doc__ = f"torch.nn.functional.{name} on the features, re-wrapped on the input's coordinates"
    return wrapped


def _loss(name):
    fn = getattr(F, name)

    def wrapped(input, target, *args, **kwargs):
        return fn(input.F, target, *args, **kwargs)
    wrapped.__name__ = wrapped.__qualname__ = name
    wrapped.__doc__ = f"torch.nn.functional.{name}(input.F, target, ...)"
    return wrapped


for _name in _FEATURE_FUNCTIONS:
    globals()[_name] = _feature_function(_name)
for _name in _LOSSES:
    globals()[_name] = _loss(_name)
del _name

__all__ = list(_FEATURE_FUNCTIONS + _LOSSES)
