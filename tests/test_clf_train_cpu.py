"""Existence-classifier training (ClassifierTrainStep, csrc/clf_train.hip) without a GPU: the new entry points are bound and
reject bad arguments before any HIP call, the step refuses CPU models, and the training oracle matches the eval oracle."""
import ctypes

import pytest
import torch

from oracle import classifier_oracle as CO
from unmore_amd.hashrng import uniform, uniform01

from clf_train_common import forward_train, param_names

NEW = ("umr_bn_train_workspace", "umr_bn_train_stats", "umr_bn_train_apply", "umr_bn_train_bwd_reduce", "umr_bn_train_bwd_apply",
       "umr_maxpool3x3s2_bwd", "umr_stuff2_add", "umr_bce_sigmoid")


def test_new_entry_points_are_bound():
    from unmore_amd import _lib
    assert set(NEW) <= set(_lib.exported_symbols())
    lib = _lib.lib()
    for name in NEW:
        assert hasattr(lib, name)


def _expect_invalid(status, what):
    from unmore_amd import _lib
    assert status == -1, (what, status)     # UMR_ERR_INVALID
    msg = _lib.lib().umr_last_error_string().decode()
    assert msg, what
    return msg


def test_argument_errors_without_a_gpu():
    from unmore_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.umr_bn_train_workspace(0, 64) == 0 and lib.umr_bn_train_workspace(100, 64) > 0
    # null pointers
    assert "null" in _expect_invalid(lib.umr_bn_train_stats(None, p, p, None, None, None, p, 16384, 16, 64, 1e-5, 0.1, 0, None), "stats")
    assert "null" in _expect_invalid(lib.umr_bn_train_apply(p, p, p, p, None, None, None, None, None, None, None, p, 16, 64, 1, 0, None), "apply")
    assert "null" in _expect_invalid(lib.umr_maxpool3x3s2_bwd(None, p, p, 1, 5, 5, 4, 0, None), "maxpool_bwd")
    assert "null" in _expect_invalid(lib.umr_stuff2_add(p, None, 1, 5, 5, 4, 0, None), "stuff2_add")
    assert "null" in _expect_invalid(lib.umr_bce_sigmoid(p, p, None, p, 4, None), "bce")
    assert "null" in _expect_invalid(lib.umr_bn_train_bwd_reduce(None, None), "bwd_reduce")
    # bad geometry
    assert "geometry" in _expect_invalid(lib.umr_bn_train_stats(p, p, p, None, None, None, p, 16384, 16, 62, 1e-5, 0.1, 0, None), "stats C")
    assert "more than one value" in _expect_invalid(lib.umr_bn_train_stats(p, p, p, p, p, None, p, 16384, 1, 64, 1e-5, 0.1, 0, None), "stats M=1")
    assert "workspace" in _expect_invalid(lib.umr_bn_train_stats(p, p, p, None, None, None, p, 4, 1000, 64, 1e-5, 0.1, 0, None), "stats ws")
    assert "geometry" in _expect_invalid(lib.umr_bn_train_apply(p, p, p, p, p, None, None, None, None, None, None, p, 16, 64, 2, 0, None), "act")
    assert "geometry" in _expect_invalid(lib.umr_maxpool3x3s2_bwd(p, p, p, 1, 0, 5, 4, 0, None), "maxpool_bwd H")
    assert "geometry" in _expect_invalid(lib.umr_stuff2_add(p, p, 1, 5, 5, 6, 0, None), "stuff2_add C")
    assert "geometry" in _expect_invalid(lib.umr_bce_sigmoid(p, p, p, p, 0, None), "bce B")
    d = _lib.BnBwdDesc()
    d.M, d.C, d.nbranch, d.dtype = 16, 64, 3, 0
    assert "geometry" in _expect_invalid(lib.umr_bn_train_bwd_apply(ctypes.byref(d), None), "bwd nbranch")
    d.nbranch = 1
    assert "gradient source" in _expect_invalid(lib.umr_bn_train_bwd_reduce(ctypes.byref(d), None), "bwd source")
    d.dy = p
    assert "null branch" in _expect_invalid(lib.umr_bn_train_bwd_reduce(ctypes.byref(d), None), "bwd branch")
    # a wrong dtype is refused too
    assert _expect_invalid(lib.umr_stuff2_add(p, p, 1, 5, 5, 4, 7, None), "dtype") == "dtype"


def test_step_refuses_a_cpu_model():
    from unmore_amd import ClassifierTrainStep
    from unmore_amd.binary_classifier import Binary_Classifier
    net = Binary_Classifier(device="cpu", image_size=64, args=None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ClassifierTrainStep(net)


def test_train_oracle_in_eval_form_is_the_eval_oracle():
    """forward_train's graph with BatchNorm in eval form is the eval oracle (CO.forward, pinned by the reference fixtures) to
    float64 rounding; in training form the same graph normalises with the batch statistics (a different answer), moves every
    running mean by momentum and counts one batch in each of the 53 BatchNorms."""
    sd = CO.hash_state("clf", uniform)
    x = torch.from_numpy(uniform01("img:clf_train_cpu", (2, 3, 64, 64))).double()
    sdd = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    want = CO.forward(sdd, x)
    got = torch.sigmoid(forward_train(dict(sdd), x, training=False))
    torch.testing.assert_close(got, want, rtol=0, atol=1e-12)
    assert all(int(sdd[n]) == 0 for n in sdd if n.endswith("num_batches_tracked"))
    logit = forward_train(dict(sdd), x)
    assert logit.shape == (2, 1) and torch.isfinite(logit).all()
    assert (torch.sigmoid(logit) - want).abs().max().item() > 1e-3
    assert all(int(sdd[n]) == 1 for n in sdd if n.endswith("num_batches_tracked"))
    assert sum(1 for n in sdd if n.endswith("num_batches_tracked")) == 53
    moved = [n for n in sdd if n.endswith("running_mean") and not torch.equal(sdd[n], sd[n].double())]
    assert len(moved) == 53
    assert len(param_names()) == 163
    assert sum(int(torch.tensor(s).prod()) for n, s in CO.state_dict_spec() if n in set(param_names())) == 25558033
