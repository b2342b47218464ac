"""ClassifierTrainStep.evaluate on the MI355X: the reference's evaluate_classification (train_objectness_net.py:703-743) counts
what the existing eval forward predicts, restores the model's mode, and leaves everything the step owns untouched."""
import pytest
import torch

from oracle import classifier_oracle as CO
from unmore_amd.hashrng import uniform, uniform01

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


def _model():
    from unmore_amd.binary_classifier import Binary_Classifier
    net = Binary_Classifier(device="cuda:0", image_size=64, args=None)
    net.load_state_dict(CO.hash_state("clf", uniform), strict=True)
    return net.to(_dev()).train()


def _batch(k, B):
    x = torch.from_numpy(uniform01(f"img:clf_eval{k}", (B, 3, 64, 64))) * torch.linspace(0.5, 1.5, B).view(B, 1, 1, 1)
    y = torch.tensor([(i + k) % 2 for i in range(B)], dtype=torch.float32).view(B, 1)
    return x.to(_dev()), y.to(_dev())


def _snapshot(net, step):
    osd = step.optimizer_state_dict()
    opt = [(i, k, v.clone() if torch.is_tensor(v) else v) for i, s in osd["state"].items() for k, v in s.items()]
    return {k: v.clone() for k, v in net.state_dict().items()}, opt, repr(osd["param_groups"]), step.iter


def _same(a, b):
    assert a[0].keys() == b[0].keys() and all(torch.equal(a[0][k], b[0][k]) for k in a[0])
    assert len(a[1]) == len(b[1])
    for (i, k, v), (j, l, w) in zip(a[1], b[1]):
        assert (i, k) == (j, l) and (torch.equal(v, w) if torch.is_tensor(v) else v == w), (i, k)
    assert a[2] == b[2] and a[3] == b[3]


def test_hits_equal_the_eval_forward_and_nothing_moves():
    from unmore_amd import ClassifierTrainStep
    net = _model()
    step = ClassifierTrainStep(net, lr=1e-3).set_graph_mode("off")
    step.step(*_batch(0, 4))                                  # a trained state: running statistics and Adam moments are non-trivial
    batches = [_batch(1, 4), _batch(2, 3)]
    net.eval()
    with torch.no_grad():
        want = sum(int(((net(images=x) > 0.5) == y).sum().item()) for x, y in batches)
    for mode in (True, False):
        net.train(mode)
        before = _snapshot(net, step)
        hits, total = step.evaluate(iter(batches))
        assert (hits, total) == (want, 7) and isinstance(hits, int)
        assert net.training is mode
        _same(before, _snapshot(net, step))
    assert step.evaluate([]) == (0, 0)


def test_mode_is_restored_after_a_raising_batch():
    from unmore_amd import ClassifierTrainStep
    net = _model()
    step = ClassifierTrainStep(net, lr=1e-3).set_graph_mode("off")

    def batches():
        yield _batch(1, 2)
        raise KeyError("the loader broke")

    for mode in (True, False):
        net.train(mode)
        with pytest.raises(KeyError):
            step.evaluate(batches())
        assert net.training is mode
    net.train()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        step.evaluate([(torch.zeros(2, 3, 64, 64), torch.zeros(2, 1))])
    assert net.training is True


@pytest.mark.parametrize("mode", ["on", "off"])
def test_a_step_after_evaluate_is_bit_identical(mode):
    """Four steps with an evaluate() between every two of them against the same four steps without: the same loss bits and
    the same final state.  With graphs 'on', steps 3 and 4 are replays of the graph captured before / around the evaluations."""
    from unmore_amd import ClassifierTrainStep
    train = [_batch(k, 2) for k in range(4)]
    evalb = [_batch(9, 3)]
    runs = []
    for with_eval in (False, True):
        net = _model()
        step = ClassifierTrainStep(net, lr=1e-3).set_graph_mode(mode)
        losses = []
        for b in train:
            losses.append(step.step(*b).item())
            if with_eval:
                hits, total = step.evaluate(evalb)
                assert total == 3 and 0 <= hits <= 3 and net.training
        runs.append((losses, step.flat_p.clone(), [b.clone() for b in net.buffers()], step.graph_replays, step.iter))
    assert runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1], runs[1][1]) and all(torch.equal(a, b) for a, b in zip(runs[0][2], runs[1][2]))
    assert runs[0][3] == runs[1][3] == (2 if mode == "on" else 0) and runs[0][4] == runs[1][4] == 4
