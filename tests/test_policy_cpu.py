"""The device actor without a device (include/chub.h, "an actor on the device"): its enums and spec struct are one list in the header,
the device code and the ctypes binding; chub_policy_input_width gives the widths chub_policy_create would work with, and every refusal
with its message; the new source file is part of the build id; tests/policy_lib.py's definition is checked by hand on a 2 -> 2 -> 2 net
and its error bound is finite and what its formula says."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import orclib
import policy_lib as pl

ROOT = orclib.ROOT
F32 = np.float32


def chub():
    import charginghub_env_amd as m
    return m


def header():
    return open(os.path.join(ROOT, "include", "chub.h")).read()


def enum_names(text, prefix):
    body = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"enum\s*(?:\w+\s*)?\{\s*(%s\w+ = 0[^}]*)\}" % prefix, body)
    assert m, prefix
    return [n for n in re.findall(r"\b%s(\w+)" % prefix, m.group(1))]


def test_enums_and_the_spec_struct_are_one_list_in_header_device_code_and_binding():
    from charginghub_env_amd import _lib
    hdr = header()
    dev = open(os.path.join(ROOT, "charginghub-env_amd", "csrc", "chub_policy.h")).read()
    for c_prefix, d_prefix, names in (("CHUB_PIN_", "PIN_", _lib.PIN_NAMES), ("CHUB_PACT_", "PACT_", _lib.PACT_NAMES),
                                      ("CHUB_PHEAD_", "PHEAD_", _lib.PHEAD_NAMES), ("CHUB_PSQ_", "PSQ_", _lib.PSQ_NAMES),
                                      ("CHUB_PRUN_", "PRUN_", _lib.PRUN_NAMES)):
        in_header, in_device = enum_names(hdr, c_prefix), enum_names(dev, d_prefix)
        assert in_header == in_device == [n.upper() for n in names] + ["COUNT"], c_prefix
    body = hdr[hdr.index("typedef struct chub_policy_spec {"):hdr.index("} chub_policy_spec;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(int32_t|float|chub_policy_input)\s+(\w+)(?:\[(\d+)\])?;", body)
    ctype = {"int32_t": C.c_int32, "float": C.c_float, "chub_policy_input": _lib.ChubPolicyInput}
    want = [(n, ctype[t] * int(k) if k else ctype[t]) for t, n, k in fields]
    got = list(_lib.ChubPolicySpec._fields_)
    assert [n for n, _ in got] == [n for n, _ in want]
    for (n, a), (_, b) in zip(got, want):
        assert C.sizeof(a) == C.sizeof(b) and getattr(a, "_length_", 1) == getattr(b, "_length_", 1), n
    assert C.sizeof(_lib.ChubPolicySpec) == 4 + 48 + 4 + 16 + 5 * 4
    inp = re.search(r"typedef struct chub_policy_input \{([^}]*)\}", hdr).group(1)
    assert re.findall(r"\w+", inp.replace("int32_t", "")) == [n for n, _ in _lib.ChubPolicyInput._fields_]
    assert _lib.POLICY_MAX_INPUTS == _lib.POLICY_MAX_LAYERS == 4
    assert int(re.search(r"kPolicyMaxInputs = (\d+), kPolicyMaxLayers = (\d+), kPolicyMaxHidden = (\d+)", dev).group(3)) == 256


def test_the_bit_threshold_is_the_step_kernels_own():
    """one constant, four places: the step kernels, the actor kernel, the numpy definition and the host's pack_actions"""
    csrc = os.path.join(ROOT, "charginghub-env_amd", "csrc")
    step = re.search(r"constexpr float kActOnThreshold = ([-0-9.e]+)f;", open(os.path.join(csrc, "chub_kernels.hip")).read()).group(1)
    actor = re.search(r"constexpr float kPolicyOnThreshold = ([-0-9.e]+)f;", open(os.path.join(csrc, "chub_policy.hip")).read()).group(1)
    assert step == actor
    assert F32(float(step)) == pl.ON_THRESHOLD == F32(-2.0 ** -25)
    # the predicate it stands for: f32((a + 1) / 2) >= 0.5
    for a in (pl.ON_THRESHOLD, np.nextafter(pl.ON_THRESHOLD, F32(-1)), F32(0), F32(-1e-7)):
        assert (F32(F32(a + F32(1)) / F32(2)) >= F32(0.5)) == (a >= pl.ON_THRESHOLD)


def test_the_new_source_file_is_part_of_the_build_id():
    from charginghub_env_amd import _lib
    mk = open(os.path.join(ROOT, "charginghub-env_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, flags=re.M).group(1).split()
    objs = re.search(r"^OBJS := (.*)$", mk, flags=re.M).group(1).split()
    assert "chub_policy.hip" in srcs and "chub_policy.h" in srcs and "chub_policy.o" in objs
    assert "chub_gae.hip" in srcs and "chub_gae.h" in srcs and "chub_gae.o" in objs
    import inspect
    hashed = re.findall(r'"(chub_\w+\.(?:hip|cpp|h))"', inspect.getsource(_lib.source_hash))
    assert sorted(hashed + ["../../include/chub.h"]) == sorted(srcs)
    lib = chub().load_library()  # (the staleness check itself: the library was built from these sources)
    assert lib.chub_build_id().decode() == _lib.source_hash()


def widths(lib, cfg, spec):
    F, A = C.c_int32(-7), C.c_int32(-7)
    rc = lib.chub_policy_input_width(C.byref(cfg), C.byref(spec), C.byref(F), C.byref(A))
    return rc, F.value, A.value


HUBS = ([20, 25], [1, 1], [64, 64], [65, 3], [0, 7], [16, 0])


def test_input_width_over_hub_shapes_and_specs():
    m = chub()
    from charginghub_env_amd import _lib
    lib = m.load_library()
    for piles in HUBS:
        cfg = m.make_config(piles, ["fast", "slow"])
        S = sum(piles)
        D = 2 + 4 * sum(1 for p in piles if p > 0) + 3
        table = [
            (("obs",), D),
            ((("pile_obs", ("car", "soc")),), 2 * S),
            ((("station_profile", ("cars", "power", "soc_gap"), 5),), 2 * 3 * 5),
            ((("forecast", ("price", "pv"), 7),), 2 * 7),
            (("obs", ("pile_obs", ("car",)), ("station_profile", ("cars",), 1), ("forecast", ("slot",), 1)), D + S + 2 + 1),
            ((("forecast", ("slot",), 3), "obs"), 3 + D),
            (("obs", "obs"), 2 * D),
        ]
        for inputs, F in table:
            for head, A in (("piles", S + 2), ("loads", 4)):
                for hidden in ((), (1,), (33, 256), (64, 64, 16)):
                    spec = _lib.policy_spec(list(hidden) + [A], inputs, head)
                    assert widths(lib, cfg, spec) == (0, F, A), (piles, inputs, head, hidden, lib.chub_last_error())


def refused(lib, cfg, spec, code, text):
    rc, F, A = widths(lib, cfg, spec)
    msg = lib.chub_last_error()
    assert rc == code and text.encode() in msg, (rc, msg, text)
    assert (F, A) == (-7, -7), "nothing is written on a refusal"


def test_every_refusal_of_a_spec_comes_with_its_message_and_without_a_device():
    m = chub()
    from charginghub_env_amd import _lib
    lib = m.load_library()
    cfg = m.make_config([20, 25], ["fast", "slow"])
    good = lambda **kw: _lib.policy_spec(kw.pop("widths", [64, 64, 47]), **kw)
    assert widths(lib, cfg, good()) == (0, 13, 47)
    F, A = C.c_int32(), C.c_int32()
    for args in ((None, C.byref(good()), C.byref(F), C.byref(A)), (C.byref(cfg), None, C.byref(F), C.byref(A)),
                 (C.byref(cfg), C.byref(good()), None, C.byref(A)), (C.byref(cfg), C.byref(good()), C.byref(F), None)):
        assert lib.chub_policy_input_width(*args) == -1 and lib.chub_last_error() == b"null argument"
    s = good(); s.n_inputs = 0
    refused(lib, cfg, s, -1, "n_inputs: 1 .. 4")
    s = good(); s.n_inputs = 5
    refused(lib, cfg, s, -1, "n_inputs: 1 .. 4")
    s = good(); s.n_layers = 0
    refused(lib, cfg, s, -1, "n_layers: 1 .. 4")
    s = good(); s.n_layers = 5
    refused(lib, cfg, s, -1, "n_layers: 1 .. 4")
    s = good(); s.inputs[0].kind = 4
    refused(lib, cfg, s, -1, "inputs[0].kind")
    s = good(inputs=("obs", "obs")); s.inputs[1].kind = -1
    refused(lib, cfg, s, -1, "inputs[1].kind")
    # a feature block's own bad arguments, with that call's message
    s = good(inputs=(("pile_obs", ("car",)),)); s.inputs[0].fields = 0
    refused(lib, cfg, s, -1, "CHUB_PILE_*")
    s = good(inputs=(("pile_obs", ("car",)),)); s.inputs[0].fields = 1 << _lib.PILE_COUNT
    refused(lib, cfg, s, -1, "CHUB_PILE_*")
    s = good(inputs=(("station_profile", ("cars",), 8),)); s.inputs[0].param = 33
    refused(lib, cfg, s, -1, "buckets: 1 .. 32")
    s = good(inputs=(("station_profile", ("cars",), 8),)); s.inputs[0].fields = 0
    refused(lib, cfg, s, -1, "CHUB_SP_*")
    s = good(inputs=(("forecast", ("price",), 8),)); s.inputs[0].param = 97
    refused(lib, cfg, s, -1, "horizon: 1 .. 96")
    s = good(inputs=(("forecast", ("price",), 8),)); s.inputs[0].fields = 1 << _lib.FC_COUNT
    refused(lib, cfg, s, -1, "CHUB_FC_*")
    for bad in (0, 257, -3):
        refused(lib, cfg, good(widths=[64, bad, 47]), -1, "width[1]: hidden widths are 1 .. 256")
    refused(lib, cfg, good(widths=[64, 64, 46]), -1, "the head's output count, 47")
    refused(lib, cfg, good(widths=[64, 47], head="loads"), -1, "the head's output count, 4")
    refused(lib, cfg, good(widths=[4]), -1, "the head's output count, 47")
    for clip in (0.0, -1.0, float("nan")):
        refused(lib, cfg, good(normalize=True, clip=clip), -1, "clip must be > 0 with normalize")
    assert widths(lib, cfg, good(normalize=False, clip=-1.0))[0] == 0  # (clip is not read without normalize)
    s = good(); s.hidden_act = 2
    refused(lib, cfg, s, -1, "hidden_act")
    s = good(); s.head = 2
    refused(lib, cfg, s, -1, "head")
    s = good(); s.squash = -1
    refused(lib, cfg, s, -1, "squash")
    s = good(); s.normalize = 2
    refused(lib, cfg, s, -1, "normalize: 0 or 1")
    refused(lib, m.make_config([0, 0], ["fast", "slow"]), good(), -1, "station_list")
    # what does not fit the kernel's LDS: F (rounded to 2) and the widest odd hidden layer share one image, the even ones the other
    fits = good(inputs=(("pile_obs", ("car", "charge", "soc", "power", "emergency")),), widths=[256, 47])   # F = 225 -> 226 + 256 rows
    assert widths(lib, cfg, fits) == (0, 225, 47)
    refused(lib, cfg, good(inputs=(("pile_obs", None),), widths=[256, 47]), -4, "rows of LDS")                # F = 405 -> 406 + 256
    assert widths(lib, cfg, good(inputs=(("pile_obs", None),), widths=[47]))[0] == 0                          # (no hidden layer: 406 rows)
    assert widths(lib, cfg, good(inputs=(("pile_obs", None),), widths=[96, 47]))[0] == 0                      # 406 + 96
    refused(lib, cfg, good(inputs=(("pile_obs", None),), widths=[97, 47]), -4, "rows of LDS")                 # 406 + 128
    # the Python side names what it does not know before the library is asked
    with pytest.raises(ValueError):
        _lib.policy_spec([47], ("observation",))
    with pytest.raises(ValueError):
        _lib.policy_spec([47], head="pile")


def test_create_and_friends_refuse_null_arguments_before_anything_else():
    m = chub()
    lib = m.load_library()
    from charginghub_env_amd import _lib
    block = C.create_string_buffer(1 << 12)
    live = C.addressof(block)  # a stand-in that is never read: the calls below are refused first
    spec = _lib.policy_spec([47])
    h = C.c_void_p()
    assert lib.chub_policy_create(None, C.byref(spec), live, live, None, None, C.byref(h)) == -1 and lib.chub_last_error() == b"null argument"
    assert lib.chub_policy_destroy(None) == 0
    assert lib.chub_policy_set_weights(None, 0, live, live) == -1 and lib.chub_last_error() == b"null argument"
    assert lib.chub_policy_set_weights_device(None, 0, live, live, None) == -1 and lib.chub_last_error() == b"null argument"
    assert lib.chub_policy_act_device(None, None, live, 13, None, live, None, None, None) == -1 and lib.chub_last_error() == b"null argument"
    assert lib.chub_policy_act(None, None, live, live) == -1 and lib.chub_last_error() == b"null argument"
    assert lib.chub_policy_run_steps(None, None, 0, live, live, None, 0, 4, None) == -1 and lib.chub_last_error() == b"bad argument"


def test_the_definition_by_hand_on_a_2_2_2_net():
    x = np.array([[0.5, -1.0]], dtype=F32)
    W0, b0 = np.array([[1.0, 2.0], [-3.0, 0.5]], dtype=F32), np.array([0.25, -0.5], dtype=F32)
    W1, b1 = np.array([[0.5, -1.0], [2.0, 0.125]], dtype=F32), np.array([0.0, 1.0], dtype=F32)
    # layer 0: z = (0.5 - 2 + 0.25, -1.5 - 0.5 - 0.5) = (-1.25, -2.5); relu -> (0, 0); layer 1: z = b1 = (0, 1); clip -> (0, 1)
    a, bound = pl.forward(x, [(W0, b0), (W1, b1)], "relu", "clip")
    assert np.array_equal(a, [[0.0, 1.0]])
    # tanh / tanh, by the formula
    a, bound = pl.forward(x, [(W0, b0), (W1, b1)], "tanh", "tanh")
    h = np.tanh(np.array([-1.25, -2.5]))
    want = np.tanh(np.array([0.5 * h[0] - h[1], 2.0 * h[0] + 0.125 * h[1] + 1.0]))
    assert np.allclose(a[0], want, rtol=0, atol=1e-15)
    # the bound, by the formula: gamma_4 over |b| + |W| |h|, the incoming error through |W|, tanhf's few ulp at every tanh
    g = 4 * pl.U / (1 - 4 * pl.U)
    e0 = g * (np.abs(b0) + np.abs(W0) @ np.abs(x[0].astype(np.float64))) + 2 * pl.TINY + pl.TANH_ERR
    held = np.abs(h) + e0
    e1 = g * (np.abs(b1) + np.abs(W1) @ held) + np.abs(W1) @ e0 + 2 * pl.TINY + pl.TANH_ERR
    assert np.allclose(bound[0], e1, rtol=1e-12, atol=0)
    assert np.isfinite(bound).all() and (bound > 0).all() and bound.max() < 1e-5
    # the bits: the predicate on the squashed f32 value, bits from S up zero
    acts = np.array([[0.0, -1e-9, -1e-7, 1.0, -1.0, pl.ON_THRESHOLD, 0.5]], dtype=F32)
    assert pl.pile_bits(acts, 6)[0, 0] == 0b101011 and pl.pile_bits(acts, 7)[0, 0] == 0b1101011
    on = np.ones((2, 130), dtype=F32)
    assert pl.pile_bits(on, 130).tolist() == [[2 ** 64 - 1, 2 ** 64 - 1, 3]] * 2
    assert np.array_equal(pl.unpack_bits(pl.pile_bits(acts, 7), 7)[0], [1, 1, 0, 1, 0, 1, 1])
    assert pl.decided([[0.0, -2.0 ** -25]], np.array([[1e-9, 1e-9]])).tolist() == [[True, False]]


def test_normalisation_is_f32_and_the_bound_is_finite_on_the_tests_distributions():
    rs = np.random.RandomState(0)
    x = rs.normal(size=(64, 13)).astype(F32) * F32(30)
    mean, inv_std = rs.normal(size=13).astype(F32), (1 / rs.uniform(0.5, 40, size=13)).astype(F32)
    y = pl.normalise(x, mean, inv_std, 5.0)
    assert y.dtype == F32 and np.abs(y).max() <= 5.0 and (np.abs(y) == 5.0).any()
    want = np.clip(((x.astype(np.float64) - mean).astype(F32).astype(np.float64) * inv_std).astype(F32), -5, 5)
    assert np.array_equal(y, want)
    left_out = []
    for sizes in ([13, 64, 64, 47], [13, 33, 33, 4], [64, 16, 1, 64, 130]):
        layers = [((rs.normal(size=(o, i)) / np.sqrt(i)).astype(F32), (rs.normal(size=o) * 0.1).astype(F32)) for i, o in zip(sizes[:-1], sizes[1:])]
        a, bound = pl.forward(rs.normal(size=(512, sizes[0])).astype(F32), layers)
        assert np.isfinite(bound).all() and bound.max() < 1e-3, sizes  # (worst case through |W| three times: ~1e-4)
        left_out.append(1.0 - pl.decided(a, bound).mean())
    assert max(left_out) < 0.01, left_out  # (the GPU test's condition on the share of bits the bound cannot decide)
    # exact data is exact: the check the GPU test relies on
    layers = pl.exact_layers(rs, [148, 256, 256, 256, 130])
    x = pl.exact_obs(rs, 32, 148)
    pl.assert_exact(x, layers)
    a, _ = pl.forward(x, layers, "relu", "clip")
    assert np.array_equal(a, a.astype(F32).astype(np.float64))
    with pytest.raises(AssertionError):
        pl.assert_exact(x * F32(4096), pl.exact_layers(rs, [148, 256, 256, 256, 130], nonzeros=64))
