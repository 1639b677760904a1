"""The critic without a device (include/chub.h, "a critic on the device"): tests/critic_lib.py's restatement against torch-CPU f64
autograd of 0.5 * mse and of PPO2's clipped value loss, the conditions on the GPU test's cases under which its bar means something (the
bar small against the gradient, every deliberate mistake outside it, no row on the predicate's edge), the exact cases' exactness, and
chub_critic_plan: counts, the fit rule at its boundary, the workgroup rule, every refusal with its code and message."""
import ctypes as C

import numpy as np
import pytest

import critic_lib as cl

F32 = np.float32
CASES = cl.gpu_general_cases()


def autograd(c):
    """the header's loss in torch f64 over nn.Linear layers -> gW, gb, v, the mean loss.  The clip range and the branch of the maximum
    are the f32 chain's (the restatement's own predicate decides ties nowhere: the cases keep away from them)"""
    import torch

    from charginghub_env_amd import wrappers

    t64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    n_rows = len(c.x)
    idx = np.arange(n_rows) if c.rows is None else np.asarray(c.rows)
    idx = idx[(idx >= 0) & (idx < n_rows)]
    lin = []
    for W, b in c.layers:
        m = torch.nn.Linear(W.shape[1], W.shape[0]).double()
        with torch.no_grad():
            m.weight.copy_(t64(W))
            m.bias.copy_(t64(b))
        lin.append(m)
    x = torch.tensor(c.x[idx])
    if c.norm is not None:
        x = wrappers.normalize_features(x, torch.tensor(c.norm[0]), torch.tensor(c.norm[1]), c.norm[2])  # (f32, as the kernel)
    h = x.double()
    for l, m in enumerate(lin):
        h = m(h)
        if l < len(lin) - 1:
            h = torch.tanh(h) if c.act == "tanh" else torch.relu(h)
    v = h[:, 0]
    ret = t64(c.ret[idx])
    if c.loss == "mse":
        terms = 0.5 * (v - ret) ** 2
    else:
        eps = float(F32(c.clip_eps))
        v_old = t64(c.v_old[idx])
        v_c = v_old + torch.clamp(v - v_old, -eps, eps)
        terms = 0.5 * torch.maximum((v - ret) ** 2, (v_c - ret) ** 2)
    loss = terms.sum() / c.R  # (1 / R with R the call's rows, skipped ones included, as the header says)
    loss.backward()
    return [m.weight.grad.numpy() for m in lin], [m.bias.grad.numpy() for m in lin], v.detach().numpy(), float(loss.detach())


def close(a, b, rel=1e-10):
    scale = max(np.abs(b).max(), 1e-300)
    return np.abs(a - b).max() <= rel * scale


AUTOGRAD_CASES = [cl.synthetic_case(F, hidden, act, 37, loss, norm, seed=100 + k)
                  for k, (F, hidden, act, loss, norm) in enumerate([
                      (45, (33, 17), "tanh", "mse", False), (45, (33, 17), "relu", "mse", True), (45, (33, 17), "tanh", "clipped", True),
                      (45, (33, 17), "relu", "clipped", False), (13, (9,), "relu", "clipped", False), (13, (), "tanh", "clipped", False)])]


@pytest.mark.parametrize("c", AUTOGRAD_CASES, ids=lambda c: c.name)
def test_the_restatement_is_autograd(c):
    """both losses, both activations, with and without the normaliser: gradients, values and the mean loss to 1e-10 relative
    (test_policy_grad_cpu's own figure for the same comparison); a minibatch by rows with a repeat and two indices outside too"""
    for rows in (None, np.array([5, 0, 36, 5, 17, -1, 18, 19, 37, 2], dtype=np.int64)):
        cc = cl.separate(c.copy(rows=rows))
        r = cl.restate(cc)
        gW, gb, v, loss = autograd(cc)
        for l in range(len(cc.layers)):
            assert close(r["gW"][l], gW[l]) and close(r["gb"][l], gb[l]), l
        assert close(r["values"][r["ok"]], v)
        # the restatement's loss terms come from f32 squares under the clipped loss (the header's): one f32 rounding per row
        tol = 1e-10 if cc.loss == "mse" else 2.0 ** -23
        assert abs(r["stats"][1] / cc.R - loss) <= tol * max(abs(loss), 1.0)
        assert r["stats"][0] == (37 if rows is None else 8)
        if cc.loss == "clipped" and rows is None:
            assert 0 < r["stats"][2] < cc.R  # some rows clipped away, some not
        else:
            assert cc.loss == "clipped" or r["stats"][2] == 0


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_the_bar_is_small_and_hides_no_mistake(c):
    """on the twin of every general GPU case: the bar below 2^-8 of each layer's largest gradient, no |d| within 1e-3 of eps, no
    candidate row with e1 - e2 inside its own derived error, and each deliberate mistake outside the bar"""
    tpw = cl.tiles_per_workgroup(c)
    r = cl.restate(c, tpw)
    cl.check_conditions(c, r)
    for m in cl.mistakes_of(c):
        assert cl.outside_bar(r, cl.restate(c, tpw, mistake=m)), m
    if c.loss == "clipped":
        eps = float(F32(c.clip_eps))
        inside, cand = np.abs(r["d"]) < eps, np.abs(r["d"]) >= eps
        assert inside.sum() > 10 and (cand & r["active"]).sum() > 10 and (cand & ~r["active"]).sum() > 10  # rows on every side of the predicate


@pytest.mark.parametrize("n_layers,hidden", [(1, cl.EXACT_HIDDEN), (2, cl.EXACT_HIDDEN), (3, cl.EXACT_HIDDEN), (4, cl.EXACT_HIDDEN), (3, cl.EXACT_WIDE)])
def test_the_exact_cases_are_exact(n_layers, hidden):
    """every R of the GPU test under both losses: dyadic data whose partial sums stay below 2^23 quanta (asserted inside), a gradient that
    says something, rows on both sides of the predicate; the wide net has more dW tiles than a workgroup keeps in registers"""
    rc, p, msg = cl.plan(cl.EXACT_F, list(hidden[:n_layers - 1]) + [1], 300, "relu")
    assert rc == 0 and (p["in_registers"] == 0) == (hidden == cl.EXACT_WIDE), msg
    for R in cl.EXACT_R:
        for loss in ("mse", "clipped"):
            c = cl.exact_case(n_layers, R, loss, hidden=hidden)
            gW, gb, v, stats = cl.exact_expected(c)
            assert all(np.isfinite(g).all() for g in gW)
            if R > 32:
                assert (gW[0] != 0).any() and (gb[-1] != 0).any()
                if loss == "clipped":
                    assert 0 < stats[2] < R


# ---- chub_critic_plan
def test_plan_counts():
    rc, p, msg = cl.plan(13, [64, 64, 1], 65536 * 96)
    assert rc == 0, msg
    assert p["n_params"] == 64 * 14 + 64 * 65 + 65
    assert p["lds_rows"] == 32 + 64 + 64 + 2 * 64 + 16 == 304 and p["lds_bytes"] == p["lds_rows"] * 33 * 4
    assert p["workgroups"] == 512 and p["in_registers"] == 1  # 2 + 4 + 2 dW tiles
    rc, q, msg = cl.plan(13, [64, 64, 1], 33)
    assert rc == 0 and q["workgroups"] == 8 and q["workspace_bytes"] < p["workspace_bytes"]
    rc, p, msg = cl.plan(64, [256, 224, 1], 4096)
    assert rc == 0, msg
    assert p["lds_rows"] == 64 + 256 + 224 + 2 * 256 + 16 and 64 * 1024 < p["lds_bytes"] <= 160 * 1024 and p["in_registers"] == 0
    assert p["n_params"] == 256 * 65 + 224 * 257 + 225
    rc, p, msg = cl.plan(1, [1], 1)
    assert rc == 0 and p["n_params"] == 2 and p["lds_rows"] == 32 + 2 * 32 + 16, msg
    rc, p, msg = cl.plan(512, [1], 1)
    assert rc == 0 and p["n_params"] == 513, msg


def test_plan_workgroup_rule():
    """ceil(R / 32) rounded up to 8, at most 512"""
    for R, want in ((1, 8), (33, 8), (32 * 8 + 1, 16), (32 * 512 + 1, 512)):
        rc, p, msg = cl.plan(13, [64, 64, 1], R)
        assert rc == 0 and p["workgroups"] == want, (R, p, msg)


def test_plan_fit_rule_at_its_boundary():
    """rows = 32 + 256 + 256 + 32 ceil(w / 32) + 2 * 256 + 16, 33 floats each, at most 160 KiB = 1241 rows: w = 160 is the last width that
    fits, 161 the first that does not"""
    rc, p, msg = cl.plan(13, [256, 256, 160, 1], 64)
    assert rc == 0 and p["lds_rows"] == 1232 and p["lds_bytes"] <= 160 * 1024, msg
    rc, p, msg = cl.plan(13, [256, 256, 161, 1], 64)
    assert rc == -4 and "LDS" in msg and "1264" in msg, (rc, msg)
    rc, p, msg = cl.plan(512, [256, 256, 1], 64)
    assert rc == -4 and "LDS" in msg, (rc, msg)


def test_plan_refusals():
    import charginghub_env_amd as chub
    from charginghub_env_amd import _lib

    for args, word in (((13, [64, 1], 0), "R is at least 1"), ((13, [64, 1], -5), "R is at least 1"), ((0, [64, 1], 64), "F: 1 .. 512"),
                       ((513, [64, 1], 64), "F: 1 .. 512"), ((13, [], 64), "n_layers"), ((13, [8, 8, 8, 8, 1], 64), "n_layers"),
                       ((13, [64, 2], 64), "must be 1"), ((13, [300, 1], 64), "hidden widths"), ((13, [0, 1], 64), "hidden widths"),
                       ((13, [64, 1], 64, 7), "hidden_act"), ((13, [64, 1], 64, "tanh", True, 0.0), "clip must be > 0"),
                       ((13, [64, 1], 64, "tanh", True, float("nan")), "clip must be > 0")):
        rc, p, msg = cl.plan(*args)
        assert rc == -1 and word in msg, (args, rc, msg)
    assert cl.plan(13, [64, 1], 64, "relu", True, 5.0)[0] == 0
    lib = chub.load_library()
    assert lib.chub_critic_plan(None, 64, None) == -1 and "null" in lib.chub_last_error().decode()
    assert lib.chub_critic_create(None, None, None, None, None, None, 64, None) == -1
    assert lib.chub_critic_destroy(None) == 0
    assert lib.chub_critic_set_weights(None, 0, None, None) == -1 and lib.chub_critic_set_weights_device(None, 0, None, None, None) == -1
    assert lib.chub_critic_set_normalizer(None, None, None) == -1 and lib.chub_critic_set_normalizer_device(None, None, None, None) == -1
    assert lib.chub_critic_normalizer_from_moments_device(None, None, 1e-8, None) == -1
    assert lib.chub_critic_values_device(None, None, 13, 1, None, 1, None, None) == -1
    assert lib.chub_critic_grad_device(None, None, None, None) == -1
    assert _lib.VLOSS == {"mse": 0, "clipped": 1} and _lib.value_loss("clipped") == 1
    with pytest.raises(ValueError):
        _lib.value_loss("huber")


def test_the_binding_matches_the_header():
    import re

    from charginghub_env_amd import _lib

    hdr = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "chub.h")).read()
    for fn in ("chub_critic_plan", "chub_critic_create", "chub_critic_destroy", "chub_critic_set_weights", "chub_critic_set_weights_device",
               "chub_critic_set_normalizer", "chub_critic_set_normalizer_device", "chub_critic_normalizer_from_moments_device",
               "chub_critic_values_device", "chub_critic_grad_device"):
        assert fn in _lib.EXPORTED and re.search(r"\bint %s\(" % fn, hdr), fn
    assert C.sizeof(_lib.ChubCriticSpec) == 36 and C.sizeof(_lib.ChubCriticGradIn) == 64 and C.sizeof(_lib.ChubCriticGradOut) == 80
