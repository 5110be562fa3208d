"""L1 Auto-PGD on the CPU side: the float64 projection against a bisection, schedule, k_sel, refusals, CLI, Predictor;
``apgd_l1_step_reference`` against the per-image oracle of tests/apgd_l1_ref.py on every operand set of the GPU test,
the census of those operands as conditions, and one proof per deliberate mistake that ``check_launch`` catches it."""
import collections
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import apgd_l1_ref as R
from attr_ref import trained_net
from pytorch_mnist_ddp_amd.data.datasets import MNIST_STD, normalize_u8
from pytorch_mnist_ddp_amd.data.synthetic import generate
from pytorch_mnist_ddp_amd.inference import Predictor, auto_pgd_l1_line, build_predict_parser
from pytorch_mnist_ddp_amd.ops import functional as Fk

LO, HI = R.LO, R.HI


@pytest.mark.parametrize("eps", [0.0, 0.5, 10.0 / MNIST_STD, 200.0])
def test_projection_against_the_bisection(eps):
    case = R.make_case(20, seed=11, eps=eps)                 # free and binding caps, a flat background, zeros, ties
    x0 = case["x0"].double()
    z = (case["x"].double() - x0) * 3.0 + case["dx"].double().sign() * torch.linspace(0, 2, 20).view(20, 1).double()
    z[0] = (case["x"][0].double() - x0[0]) * 0.2             # well inside for eps >= 0.5
    delta, lam = Fk.l1_box_projection_reference(z, x0, eps, LO, HI)
    for i in range(20):
        want, lam_w, unique = R.project(z[i].numpy(), x0[i].numpy(), eps)
        assert unique
        assert np.abs(delta[i].numpy() - want).max() <= 1e-12 and abs(float(lam[i]) - lam_w) <= 1e-12, i
    p = x0 + delta
    assert (delta.abs().sum(dim=1) <= eps * (1 + 1e-12)).all() and (p >= LO).all() and (p <= HI).all()
    assert torch.equal(p, x0) if eps == 0.0 else (float(lam[0]) == 0.0 and torch.equal(delta[0], z[0]))  # inside: untouched


def test_checkpoints_and_k_sel():
    assert Fk.apgd_l1_checkpoints(100) == tuple((i, 4) for i in range(4, 101, 4))
    assert Fk.apgd_l1_checkpoints(50) == tuple((i, 2) for i in range(2, 51, 2))
    assert Fk.apgd_l1_checkpoints(10)[0] == (1, 1) and Fk.apgd_l1_checkpoints(110)[-1] == (108, 4)
    assert [Fk.apgd_l1_k_sel(sp) for sp in (0, 1, 2, 3, 784)] == [1, 1, 2, 2, 523]


def test_refusals_of_the_new_entry_points():
    z, f, n = torch.zeros(2, 784), torch.zeros(2, 4), torch.zeros(2, 4, dtype=torch.int32)
    for bad in (dict(sign=0), dict(eps=-1.0), dict(first=True, last=True), dict(window=-1)):
        with pytest.raises(ValueError):
            Fk.apgd_l1_step_reference(z, torch.zeros(2), z, z, z, z, f, n, **dict(dict(sign=1, eps=1.0, lo=LO, hi=HI), **bad))
    pr, x = Predictor(trained_net()), torch.zeros(2, 1, 28, 28)
    for kw in (dict(eps=-1.0), dict(steps=0), dict(loss="l1"), dict(targeted=True), dict(labels=torch.tensor([0]))):
        with pytest.raises(ValueError):
            pr.auto_pgd_l1(x, **kw)


def test_predict_parser_and_line():
    d = build_predict_parser().parse_args([])
    assert (d.apgd_eps, d.apgd_steps, d.apgd_norm, d.apgd_restarts, d.apgd_seed, d.apgd_loss) == (None, 100, "linf", 1, 0, "ce")
    assert (d.apgd_l1_eps, d.apgd_l1_steps, d.apgd_l1_loss) == (None, 100, "ce")
    assert auto_pgd_l1_line(10, 100, 0.12344, 9876, 10000, 23.5) == \
        "Auto-PGD set (L1 eps=10, steps=100): Average loss: 0.1234, Accuracy: 9876/10000 (99%), median pixels changed: 23.5"
    line = auto_pgd_l1_line(5, 3, 1.0, 1, 2, None, "cw")
    assert line.startswith("Auto-PGD set (L1 eps=5, steps=3, loss=cw): ") and line.endswith("median pixels changed: n/a")


def test_predictor_auto_pgd_l1_cpu():
    imgs, labels = generate(64, seed=5)
    x0, y = normalize_u8(imgs).reshape(64, 784)[:8], labels[:8].long()
    pr = Predictor(trained_net())
    x_adv, lp, loss_best = pr.auto_pgd_l1(x0.view(8, 1, 28, 28), y, eps=10.0, steps=10)
    xa = x_adv.reshape(8, 784)
    mass = (xa.double() - x0.double()).abs().sum(dim=1)
    assert (xa >= LO).all() and (xa <= HI).all() and (mass <= 10.0 / MNIST_STD * (1 + 1e-5)).all()
    start = F.nll_loss(pr.log_probs(x0.view(8, 1, 28, 28)), y, reduction='none')
    assert (loss_best >= start).all() and float(mass.max()) > 1.0
    assert torch.allclose(F.nll_loss(lp, y, reduction='none'), loss_best, atol=1e-5)


@functools.lru_cache(maxsize=None)
def _sets():
    """Every operand set of the GPU test with its oracle, census and float32 reference, computed once."""
    out = []
    for name, case, kw, group in R.launch_sets():
        info = []
        out.append((name, case, kw, group, (R.step_oracle(case, info=info, **kw), info), R.reference_launch(case, **kw)))
    return out


def test_reference_against_the_oracle():
    """float32: everything discrete bit for bit, NaN where the oracle's are, lam under the bound derived from the
    suffix sum (apgd_l1_ref's docstring), x under that bound + its own roundings; float64: the oracle to 1e-9."""
    worst_lam = worst_x = 0.0
    for name, case, kw, group, (want, info), ref in _sets():
        bad = R.check_launch(ref, case, kw, ref, oracle=(want, info))
        assert bad == [], (name, bad)                        # (the scaled rules hold trivially: got is ref)
        assert R.check_launch(R.rounded(want), case, kw, ref, oracle=(want, info)) == [], name   # the oracle, rounded once
        ref64 = R.reference_launch(case, torch.float64, **kw)
        for i, rec in enumerate(info):
            ok = ~np.isnan(want[0][i])
            assert np.abs(ref64[0][i] - want[0][i])[ok].max(initial=0.0) <= 1e-9, (name, i)
            if rec["path"] != "sort" or not rec["unique"]:
                continue
            assert abs(ref64[3][i, 2] - want[3][i, 2]) <= 1e-9, (name, i)
            dl = abs(float(ref[3][i, 2]) - want[3][i, 2])
            dx = np.abs(ref[0][i].astype(np.float64) - want[0][i]) / (rec["lam_bound"] + rec["x_bound"])
            assert dl <= rec["lam_bound"] < 1e-3 * case["eps"] and dx.max() <= 1.0, (name, i, dl, rec["lam_bound"])
            worst_lam, worst_x = max(worst_lam, dl / rec["lam_bound"]), max(worst_x, float(dx.max()))
    print(f"\nfloat32 reference: largest lam deviation / derived bound {worst_lam:.4f}, x {worst_x:.4f}")


def test_census_conditions():
    seeded, hand = collections.Counter(), collections.Counter()
    for name, case, kw, group, (want, info), ref in _sets():
        for i, rec in enumerate(info):
            (hand if group else seeded).update(R.branches(rec))
            flat = group is not None and i in group["flat"]
            assert rec["unique"] != flat, (name, i)          # lam is left uncompared on the named flat images only
        if name.startswith("kind-") and name.endswith("-1") and name.split("-")[1] in ("free", "caps", "partial"):
            assert info[0]["path"] == "sort", name           # M = 1 reaches the projection's sort
        if "partial" in name:
            for rec in info:
                assert rec["path"] == "sort" and 4 * rec["partial_sel"] >= rec["m"] and rec["crossing"] in "ab", name
    assert [b for b in R.BRANCHES if seeded[b] < 3] == [] and [b for b in R.BRANCHES if hand[b] < 1] == []
    print("\ncensus, seeded:", dict(seeded), "\ncensus, hand:", dict(hand))


def test_hand_images_take_their_branches():
    g = R.hand_case()
    info = R.census(g["checkpoint"]["case"], window=2)
    rows = [(sp, old, form) for sp, old in R.RESTART_PAIRS for form in ("stored", "improved")]
    for rec, (sp, old, form) in zip(info, rows):
        assert rec["restart"] == (100 * sp < 95 * old) and rec["improved"] == (form == "improved")
    assert [rec["restart"] for rec in info[::2][:8]] == [True, False, False, True, False, False, True, False]
    assert [rec["k_sel"] for rec in info[16:20]] == [1, 2, 2, 523] and info[10]["k_sel"] == 1       # sp = 1, 2, 3, 784; 0
    eta = R.step_oracle(g["checkpoint"]["case"], window=2)[3][-3:, 0]
    assert eta.tolist() == [4.0, 3.0, 3.0] and [rec["floor"] for rec in info[-3:]] == [False, True, True]
    info, lab = R.census(g["plain"]["case"]), g["plain"]["labels"]
    at = lambda name: info[lab.index(name)]                                                   # noqa: E731
    assert (at("ties")["m"], at("all_equal")["m"], at("few_nonzero")["m"], at("zero_grad")["m"]) == (261, 784, 49, 0)
    assert at("neg_zero_denormal")["m"] == 250 and 0 < at("neg_zero_denormal")["thr_bits"] < 1 << 23   # a denormal
    assert at("huge_among_denormals")["m"] == 3 and at("alt64")["m"] == 384 and at("alt256")["m"] == 272
    want = R.step_oracle(g["plain"]["case"])
    assert want[3][lab.index("exact"), 2] == pytest.approx(0.25, abs=1e-15) and at("exact")["unique"]
    assert not at("flat")["unique"] and at("flat")["partial"] == 16 and at("b_crossing")["crossing"] == "b"
    assert at("equal_breakpoints")["crossing"] == "a" and at("zero_grad")["path"] == "inside"
    j = lab.index("outside_box")
    assert (want[0][j, :3] == HI).all() and (want[0][j, 3:6] == LO).all()                      # cap 0, then the clamp
    assert want[4][-4:, 0].tolist() == [0, -5, 785, 1 << 30] and [r["m"] for r in info[-4:]] == [1, 1, 784, 784]
    for name, nan_x in (("nan_plain", 784), ("nan_restart", 784), ("nan_eps0", 1)):
        c, kw, at_ = g[name]["case"], g[name]["kw"], g[name]["nan"][-1]
        want, clean = R.step_oracle(c, **kw), R.step_oracle(g[name]["clean"], **kw)
        assert np.isnan(want[0][at_]).sum() == nan_x and np.isnan(want[3][at_, 2]) == (nan_x == 784)
        assert all(np.array_equal(w[[0, 3]], k[[0, 3]]) for w, k in zip(want, clean))          # the NaN stays in its image
        if name != "nan_restart":                            # the NaN loss: not the best, the image moves as without it
            assert want[3][1, 1] == c["fstate"][1, 1] and not np.isnan(want[0][1]).any()
            assert np.array_equal(want[1][1], c["x_best"][1].numpy())


# what catches each mistake: "old" - the bit-for-bit and launch-wide rules on the 36 seeded cases; "hand" - those rules
# on the hand-made images only; "image" - nothing but the per-image lam and per-element x rules
CAUGHT_BY = dict(ball_then_clamp="old", cap_wrong_side="old", thr_next="old", ties_cut="old", zeros_selected="hand",
                 m_is_k_sel="old", sp_on_x="old", restart_le="old", k_sel_floor="old", no_eta_floor="old",
                 restart_dx="old", sp_old_kept="old", lam_neighbour="old", nan_loss_best="hand", restarted_kept="old",
                 lam_offset="image", crossing_n_ge0=None, pick_strict=None)


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_every_mutation_is_caught(variant):
    """The oracle with one deliberate mistake, rounded to float32 as a kernel would store it, fails ``check_launch``
    (the unmutated one passes on every set: ``test_reference_against_the_oracle``).  The two of ``R.EQUIVALENT`` are
    findings, not proofs: N_k > 0 holds at the first crossing in exact arithmetic (phi falls strictly into it), and
    the segments on either side of a breakpoint give the same lam there, so ``<`` for ``<=`` only moves lam along a
    flat piece, where it is not compared; no operand of these tests tells them from the rule."""
    where = collections.defaultdict(set)
    for name, case, kw, group, oracle, ref in _sets():
        got = R.rounded(R.step_oracle(case, variant=variant, **kw))
        rules = {rule for rule, _ in R.check_launch(got, case, kw, ref, oracle=oracle)}
        if variant in R.EQUIVALENT:
            assert rules == set(), name
        if rules & {"discrete", "launch", "box", "nan"}:
            where["hand" if group else "old" if name.startswith("seeded") else "kinds"].add(name)
        elif rules:
            where["image"].add(name)
    by = "old" if where["old"] else "hand" if where["hand"] else "image" if where["image"] else None
    print(f"\n{variant}: caught by {by}", {k: len(v) for k, v in where.items()})
    assert by == CAUGHT_BY[variant], dict(where)
    assert (variant in R.EQUIVALENT) == (by is None)


def test_the_partial_operands_catch_a_projection_without_the_b_breakpoints():
    """The kernel with its b keys left out is the ball alone, then the clamp: every ``partial`` launch fails, M = 1
    included; ``<=`` for ``<`` in ``red`` fails on the hand-made checkpoint launch."""
    for name, case, kw, group, oracle, ref in _sets():
        if "partial" in name:
            got = R.rounded(R.step_oracle(case, variant="ball_then_clamp", **kw))
            assert {r for r, _ in R.check_launch(got, case, kw, ref, oracle=oracle)} >= {"launch", "image_lam", "elem_x"}
        if name == "hand-checkpoint":
            got = R.rounded(R.step_oracle(case, variant="restart_le", **kw))
            assert ("discrete", "istate") in R.check_launch(got, case, kw, ref, oracle=oracle)
