"""Actor gradients without a device (include/chub.h, "actor gradients on the device"): tests/policy_grad_lib.py's restatement against
torch-CPU f64 autograd through the wrappers' own functions, the conditions on the GPU test's cases under which its bar means something
(the bar small against the gradient, every deliberate mistake outside it, no ratio on a clip bound), the exact cases' exactness, and
chub_policy_grad_plan: counts, the fit rule at its boundary, every refusal with its code."""
import numpy as np
import pytest

import policy_grad_lib as pgl
import policy_sample_lib as ps

F32 = np.float32
CASES = pgl.gpu_general_cases()


def autograd(c):
    """the loss of the header in torch f64 through normalize_features + nn.Linear + sampled_logp + sampled_entropy -> gW, gb, gls, logp, ent"""
    import torch

    from charginghub_env_amd import wrappers

    t64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    idx = np.arange(len(c.features)) if c.rows is None else np.asarray(c.rows)
    lin = []
    for W, b in c.layers:
        m = torch.nn.Linear(W.shape[1], W.shape[0]).double()
        with torch.no_grad():
            m.weight.copy_(t64(W))
            m.bias.copy_(t64(b))
        lin.append(m)
    log_std = t64(c.log_std).requires_grad_(True)
    x = torch.tensor(c.features[idx])
    if c.norm is not None:
        x = wrappers.normalize_features(x, torch.tensor(c.norm[0]), torch.tensor(c.norm[1]), c.norm[2])  # (f32, as the kernel)
    h = x.double()
    for l, m in enumerate(lin):
        h = m(h)
        if l < len(lin) - 1:
            h = torch.tanh(h) if c.act == "tanh" else torch.relu(h)
    piles = c.head == "piles"
    S = c.S if piles else 0
    on = torch.tensor(c.on[idx][:, :S]) if piles else torch.zeros((len(idx), 0), dtype=torch.bool)
    st = None if (c.sets is None or not piles) else torch.tensor(c.sets[idx][:, :S])
    logp = wrappers.sampled_logp(h, on, t64(c.u[idx]), log_std, piles=st)
    ent = wrappers.sampled_entropy(h, log_std, piles=st)
    A = np.asarray(c.adv, dtype=F32)
    if c.adv_stats is not None:
        A = pgl.adv_norm(A, c.adv_stats)
    A = t64(A[idx])
    ec = float(F32(c.ent_coef))
    if c.loss == "coef":
        loss = (-A * logp - ec * ent).mean()
    else:
        ratio = torch.exp(logp - t64(c.logp_old[idx]))
        lo, hi = float(F32(1) - F32(c.clip_eps)), float(F32(1) + F32(c.clip_eps))
        loss = (-torch.minimum(ratio * A, torch.clamp(ratio, lo, hi) * A) - ec * ent).mean()
    loss.backward()
    return ([m.weight.grad.numpy() for m in lin], [m.bias.grad.numpy() for m in lin], log_std.grad.numpy(), logp.detach().numpy(), ent.detach().numpy(),
            float(loss.detach()))


def close(a, b, rel=1e-10):
    scale = max(np.abs(b).max(), 1e-300)
    return np.abs(a - b).max() <= rel * scale


AUTOGRAD_CASES = [pgl.separate_ratios(pgl.synthetic_case(piles, hidden, act, head, 37, loss, sets, norm, seed=100 + k, adv_stats=stats))
                  for k, (piles, hidden, act, head, loss, sets, norm, stats) in enumerate([
                      ([20, 25], (33, 17), "tanh", "piles", "ppo_clip", True, True, False),
                      ([20, 25], (33, 17), "relu", "piles", "ppo_clip", False, False, True),
                      ([20, 25], (33,), "tanh", "loads", "ppo_clip", False, True, False),
                      ([20, 25], (33,), "relu", "loads", "coef", False, False, True),
                      ([3, 2], (9,), "relu", "piles", "coef", True, False, False),
                      ([40, 37], (), "tanh", "piles", "ppo_clip", True, False, False)])]


@pytest.mark.parametrize("c", AUTOGRAD_CASES, ids=lambda c: c.name + "-" + c.loss)
def test_the_restatement_is_autograd_through_the_wrappers(c):
    """both losses, both heads, both activations, with and without sets, normaliser and advantage statistics: gradients, logp, entropy
    and the mean loss to 1e-10 relative; a minibatch by rows with a repeated index too"""
    for rows in (None, np.array([5, 0, 36, 5, 17, 18, 19, 2], dtype=np.int64)):
        cc = pgl.separate_ratios(c.copy(rows=rows))
        r = pgl.restate(cc)
        gW, gb, gls, logp, ent, loss = autograd(cc)
        for l in range(len(cc.layers)):
            assert close(r["gW"][l], gW[l]) and close(r["gb"][l], gb[l]), l
        assert close(r["gls"], gls) and close(r["logp"], logp) and close(r["ent"], ent)
        assert abs(r["stats"][1] / cc.R - loss) <= 1e-10 * max(abs(loss), 1.0)
        if cc.loss == "ppo_clip" and rows is None:
            assert 0 < r["stats"][4] < cc.R  # some rows clipped away, some not


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name + "-" + c.loss)
def test_the_bar_is_small_and_hides_no_mistake(c):
    """on the twin of every general GPU case: the bar below 2^-8 of each layer's largest gradient, no ratio within 1e-3 of a clip bound,
    and each deliberate mistake outside the bar"""
    tpw = pgl.tiles_per_workgroup(c.piles, list(c.hidden) + [c.layers[-1][0].shape[0]], c.R, c.head, c.act, c.inputs)
    r = pgl.restate(c, tpw)
    pgl.check_conditions(c, r)
    for m in pgl.MISTAKES:
        if (m == "set_ignored" and c.sets is None) or (m == "row_dropped" and c.R < 2) or (m == "no_1_over_R" and c.R == 1):
            continue
        assert pgl.outside_bar(r, pgl.restate(c, tpw, mistake=m)), m
    if c.loss == "ppo_clip" and c.R >= 70:
        up, down = pgl.clipped_both_ways(c, r)
        assert up >= 1 and down >= 1, (up, down)


@pytest.mark.parametrize("n_layers,hidden", [(1, (33, 64, 31)), (2, (33, 64, 31)), (3, (33, 64, 31)), (4, (33, 64, 31)), (3, pgl.EXACT_WIDE)])
def test_the_exact_cases_are_exact(n_layers, hidden):
    """every R of the GPU test: dyadic data whose partial sums stay below 2^23 quanta (asserted inside), a gradient that says something;
    the wide net has more dW tiles than a workgroup keeps in registers"""
    rc, p, msg = pgl.plan([20, 25], list(hidden[:n_layers - 1]) + [4], 300, "loads", "relu")
    assert rc == 0 and (p["in_registers"] == 0) == (hidden == pgl.EXACT_WIDE), msg
    for R in pgl.R_LIST + (300,):
        c = pgl.exact_case(n_layers, R, hidden=hidden)
        gW, gb, gls = pgl.exact_expected(c)
        assert all(np.isfinite(g).all() for g in gW) and (gW[0] != 0).any() and (gb[-1] != 0).any() and (gls != 0).all()
        if R > 32:
            assert all(len(np.unique(g)) > 4 for g in gW)


# ---- chub_policy_grad_plan
def test_plan_counts():
    rc, p, msg = pgl.plan([20, 25], [64, 64, 47], 65536 * 96)
    assert rc == 0, msg
    assert p["n_params"] == 64 * 14 + 64 * 65 + 47 * 65
    assert p["lds_rows"] == 32 + 64 + 64 + 2 * 64 + 16 and p["lds_bytes"] == p["lds_rows"] * 33 * 4
    assert p["workgroups"] == 512 and p["in_registers"] == 1  # 2 + 4 + 4 dW tiles
    rc, q, msg = pgl.plan([20, 25], [64, 64, 47], 33)
    assert rc == 0 and q["workgroups"] == 8 and q["workspace_bytes"] < p["workspace_bytes"]
    rc, q, msg = pgl.plan([20, 25], [64, 64, 47], 32 * 9)
    assert rc == 0 and q["workgroups"] == 16
    # 64 -> 256 -> 256 -> 47: fits the CU's 160 KiB, too many tiles for registers
    rc, p, msg = pgl.plan([20, 25], [256, 256, 47], 4096, inputs=("obs", ("pile_obs", ("car",)), ("forecast", ("price",), 6)))
    assert rc == 0, msg
    assert p["lds_rows"] == 64 + 256 + 256 + 2 * 256 + 16 and p["lds_bytes"] <= 160 * 1024 and p["in_registers"] == 0
    assert p["n_params"] == 256 * 65 + 256 * 257 + 47 * 257


def test_plan_fit_rule_at_its_boundary():
    """rows = 32 + 256 + 256 + 32 ceil(w / 32) + 2 * 256 + 16, 33 floats each, at most 160 KiB = 1241 rows: w = 160 fits, 161 does not"""
    rc, p, msg = pgl.plan([20, 25], [256, 256, 160, 47], 64)
    assert rc == 0 and p["lds_rows"] == 1232 and p["lds_bytes"] <= 160 * 1024, msg
    rc, p, msg = pgl.plan([20, 25], [256, 256, 161, 47], 64)
    assert rc == -4 and "LDS" in msg and "1264" in msg, (rc, msg)
    # such a policy still has a feature width and acts (the deterministic fit rule is untouched)
    import ctypes as C

    import charginghub_env_amd as chub
    from charginghub_env_amd import _lib

    cfg = _lib.ChubConfig()
    cfg.station_list[0], cfg.station_list[1] = 20, 25
    spec = _lib.policy_spec([256, 256, 161, 47])
    F, A = C.c_int32(), C.c_int32()
    assert chub.load_library().chub_policy_input_width(C.byref(cfg), C.byref(spec), C.byref(F), C.byref(A)) == 0 and (F.value, A.value) == (13, 47)


def test_plan_refusals():
    assert pgl.plan([20, 25], [64, 47], 0)[0] == -1
    assert pgl.plan([20, 25], [64, 47], -5)[0] == -1
    assert pgl.plan([20, 25], [64, 46], 64)[0] == -1          # not the head's output count
    assert pgl.plan([20, 25], [300, 47], 64)[0] == -1         # a hidden width beyond 256
    assert pgl.plan([20, 25], [64, 4], 64, head="loads")[0] == 0
    import ctypes as C

    import charginghub_env_amd as chub

    lib = chub.load_library()
    assert lib.chub_policy_grad_plan(None, None, 64, None) == -1
    assert lib.chub_policy_grad_create(None, 64, None) == -1
    assert lib.chub_policy_grad_destroy(None) == 0
    assert lib.chub_policy_grad_device(None, None, None, None) == -1
