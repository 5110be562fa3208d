"""``Predictor.carlini_wagner`` on the CPU (``reference_carlini_wagner`` over ``cw_step_reference``): the invariants
of a result, a loose sanity bound on the optimiser, the bisection table and the argument checks."""
import pytest
import torch

from pytorch_mnist_ddp_amd.inference import _PIXEL_LUT, Predictor
from pytorch_mnist_ddp_amd.ops import functional as Fk

import cw_ref as R
import deepfool_ref as D


def _case(n=8):
    imgs, _ = D.trained_case()
    labels, _ = R.cpu_carlini_wagner()
    return imgs[:n], labels[:n]


def test_reference_invariants_and_more_steps():
    imgs, labels = _case()
    pr = Predictor(D.trained_net())
    assert not pr.native
    x = _PIXEL_LUT[imgs.reshape(8, 784).long()]
    short = pr.carlini_wagner(imgs, labels, search_steps=3, steps=30)
    R.check_invariants(x, labels.long(), short, pr.predict(imgs))
    assert short[0].shape == (8, 1, 28, 28) and short[1][1] == 0 and short[3].all()
    long = pr.carlini_wagner(imgs, labels, search_steps=3, steps=60)
    R.check_invariants(x, labels.long(), long, pr.predict(imgs))
    both = short[3] & long[3]
    assert both.any() and (long[1][both] <= 1.05 * short[1][both]).all()       # loose: an optimiser, not a measurement


def test_large_c_finds_every_image_in_one_search():
    imgs, labels = _case()
    _, radii, _, found = Predictor(D.trained_net()).carlini_wagner(imgs, labels, search_steps=1, steps=30, c_init=1e4)
    assert found.all() and torch.isfinite(radii).all()


@pytest.mark.parametrize("succ,c,c_lo,c_hi,want", [
    (1, 1.0, 0.0, Fk.CW_C_INF, (0.5, 0.0, 1.0)),             # the first success: c_hi is set, c halves
    (0, 1.0, 0.0, Fk.CW_C_INF, (10.0, 1.0, Fk.CW_C_INF)),    # no success and no upper end yet: tenfold
    (0, 0.5, 0.0, 1.0, (0.75, 0.5, 1.0)),                    # no success inside a bracket: the upper half
    (1, 0.75, 0.5, 1.0, (0.625, 0.5, 0.75)),                 # a success inside a bracket: the lower half
])
def test_bisection_table(succ, c, c_lo, c_hi, want):
    z = torch.zeros(1, 784)
    out = Fk.cw_step_reference(z, torch.tensor([-1.0]), z, z, z, z, z, z, torch.tensor([[c, c_lo, c_hi, float("inf")]]),
                               torch.tensor([[succ, 0, 9, 0]], dtype=torch.int32), 1, 0.0, 0.05, 1.0, 1, 0, R.LO, R.HI,
                               search_end=True)
    assert torch.equal(out[5][0, :3], torch.tensor(want)) and out[6][0].tolist() == [0, 0, 9, 0]
    assert torch.equal(out[0], Fk.cw_w0(z, R.LO, R.HI)) and not out[1].any() and not out[2].any()


@pytest.mark.parametrize("kw", [dict(targeted=True), dict(kappa=-0.5), dict(lr=0.0), dict(search_steps=0)])
def test_argument_checks(kw):
    imgs, labels = _case(2)
    with pytest.raises(ValueError, match="carlini_wagner"):
        Predictor(D.trained_net()).carlini_wagner(imgs, None if "targeted" in kw else labels, **kw)
