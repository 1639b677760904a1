"""The training log's host-only parts (include/chub.h, "a training log and a KL stop on the device") against tests/trainlog_lib.py, without a
device: the symbols, chub_train_log_fold bit for bit over made sequences of stats blocks, chub_ppo_update's split, the refusals that need
no device, and the failure experiment on the restatement's wrong variants."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import trainlog_lib as tl

ERR_ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["chub_train_log_create", "chub_train_log_destroy", "chub_train_log_begin_device", "chub_train_log_record_device",
       "chub_train_log_steps_device", "chub_train_log_device", "chub_train_log_read", "chub_train_log_fold", "chub_adam_set_gate",
       "chub_ppo_update_plan", "chub_ppo_update"]
SEQ = tl.sequences()


def lib():
    from charginghub_env_amd import _lib
    return _lib.load_library()


def last_error():
    return lib().chub_last_error().decode()


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_the_new_symbols_are_declared_exported_and_bound():
    from charginghub_env_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "chub.h")).read()
    L = lib()
    for fn in NEW:
        assert fn in _lib.EXPORTED and re.search(r"\bint %s\(" % fn, hdr), fn
        assert getattr(L, fn).argtypes is not None, fn
    # the enums of the header, the binding's and the restatement's
    words = dict(re.findall(r"CHUB_TLOG_(\w+) = (\d+)", hdr))
    assert {k.lower(): int(v) for k, v in words.items() if k != "WORDS"} == _lib.TLOG and int(words["WORDS"]) == _lib.TLOG_WORDS == tl.WORDS
    assert (_lib.TLOG["counted"], _lib.TLOG["after_stop"], _lib.TLOG["stopped"], _lib.TLOG["stop_index"], _lib.TLOG["actor"], _lib.TLOG["kl_max"],
            _lib.TLOG["kl_last"], _lib.TLOG["critic"], _lib.TLOG["actor_opt"], _lib.TLOG["critic_opt"]) == \
           (tl.COUNTED, tl.AFTER_STOP, tl.STOPPED, tl.STOP_INDEX, tl.ACTOR, tl.KL_MAX, tl.KL_LAST, tl.CRITIC, tl.ACTOR_OPT, tl.CRITIC_OPT)
    assert re.search(r"enum \{ CHUB_KL_K1 = 0, CHUB_KL_K3, CHUB_KL_COUNT \}", hdr) and _lib.KL == {"k1": tl.K1, "k3": tl.K3}
    # the args struct is the header's, field for field
    body = re.search(r"typedef struct chub_ppo_update_args \{(.*?)\} chub_ppo_update_args;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?=,|$)", decl.strip())]
    assert names == [n for n, _ in _lib.ChubPpoUpdateArgs._fields_], names
    assert C.sizeof(_lib.ChubPpoUpdateArgs) == 192  # (24 words of 8 bytes: no padding but pad_)


def fold(seq):
    """chub_train_log_fold over the sequence's record steps from what begin leaves -> (words, gate)"""
    w = np.zeros(tl.WORDS, dtype=np.float64)
    w[tl.STOP_INDEX] = -1.0
    gate = np.zeros(1, dtype=np.int64)
    for ps, cs, _, _ in seq["blocks"]:
        assert lib().chub_train_log_fold(ptr(w), ptr(gate), ptr(ps), ptr(cs), seq["kind"], C.c_double(seq["kl_limit"])) == 0, last_error()
    return w, gate


def record_only(seq, wrong=None):
    log = tl.Log(wrong)
    for ps, cs, _, _ in seq["blocks"]:
        log.record(ps, cs, seq["kind"], seq["kl_limit"])
    return log


@pytest.mark.parametrize("name", list(SEQ))
def test_fold_equals_the_restatement_bit_for_bit(name):
    seq = SEQ[name]
    w, gate = fold(seq)
    want = record_only(seq)
    assert np.array_equal(tl.bits(w), tl.bits(want.w)), (name, w, want.w)
    assert gate[0] == want.gate
    # what the sequence was made to show
    stopped_at = None if w[tl.STOP_INDEX] < 0 else int(w[tl.STOP_INDEX])
    assert (stopped_at, int(w[tl.COUNTED]), int(w[tl.AFTER_STOP])) == (seq["stopped_at"], seq["counted"], seq["after_stop"]), name
    assert w[tl.STOPPED] == gate[0] == (seq["stopped_at"] is not None)
    assert (w[tl.ACTOR_OPT:] == 0).all(), "the record step leaves the optimisers' words alone"


def test_the_sums_hold_the_counted_minibatches_only():
    seq = SEQ["below-below-above-below"]
    w, _ = fold(seq)
    ps = [b[0] for b in seq["blocks"]]
    cs = [b[1] for b in seq["blocks"]]
    assert np.array_equal(tl.bits(w[tl.ACTOR:tl.ACTOR + 6]), tl.bits((ps[0] + ps[1]) + ps[2]))
    assert np.array_equal(tl.bits(w[tl.CRITIC:tl.CRITIC + 6]), tl.bits((cs[0] + cs[1]) + cs[2]))
    assert w[tl.KL_MAX] == w[tl.KL_LAST] == ps[2][3] / ps[2][0] > seq["kl_limit"]


def test_k1_and_k3_disagree_on_the_pair():
    """the same blocks: at index 1 only K3 passes the limit, at index 2 only K1"""
    blocks = SEQ["k1-of-the-pair"]["blocks"]
    log = tl.Log()
    k1 = [log.kl(b[0], tl.K1) for b in blocks]
    k3 = [log.kl(b[0], tl.K3) for b in blocks]
    assert k1[1] < 0.03 < k3[1] and k3[2] < 0.03 < k1[2], (k1, k3)
    assert fold(SEQ["k1-of-the-pair"])[0][tl.STOP_INDEX] == 2 and fold(SEQ["k3-of-the-pair"])[0][tl.STOP_INDEX] == 1


def test_a_log_by_hand():
    """two minibatches and a stop, every number written out"""
    log = tl.Log()
    log.record([4.0, 8.0, 2.0, 1.0, 1.0, 5.0], [4.0, 2.0, 0.0, 1.0, 2.0, 3.0], tl.K3, 1.0)
    # K3 = (5 / 4 - 1) + 1 / 4 = 0.5
    assert list(log.w[:4]) == [1, 0, 0, -1] and log.w[tl.KL_MAX] == log.w[tl.KL_LAST] == 0.5 and log.gate == 0
    log.record([4.0, 0.0, 0.0, 8.0, 0.0, 4.0], None, tl.K3, 1.0)  # K3 = 0 + 2
    assert list(log.w[:4]) == [2, 0, 1, 1] and log.w[tl.KL_MAX] == 2.0 and log.gate == 1 and log.w[tl.ACTOR + 3] == 9.0 and log.w[tl.CRITIC] == 4.0
    log.record([4.0, 0.0, 0.0, 0.0, 0.0, 4.0], None, tl.K3, 1.0)
    assert list(log.w[:4]) == [2, 1, 1, 1] and log.w[tl.KL_LAST] == 2.0 and log.w[tl.ACTOR] == 8.0
    log.steps([3.0, 2.0, 0.5, 0.0], [3.0, np.inf, 0.0, 1.0])
    log.steps([3.0, 4.0, 0.0, 2.0], [3.0, 1.0, 1.0, 0.0])
    assert list(log.w[tl.ACTOR_OPT:tl.ACTOR_OPT + 6]) == [1, 0, 1, 6.0, 4.0, 1] and list(log.w[tl.CRITIC_OPT:]) == [1, 1, 0, 1.0, 1.0, 0]


@pytest.mark.parametrize("mb,want", [(100, (4, 84)), (384, (1, 384)), (385, (1, 384)), (1, (384, 1))])
def test_the_split_of_384_rows(mb, want):
    from charginghub_env_amd import vec_env
    assert vec_env.ppo_update_plan(384, mb) == want == tl.split(384, mb)


def test_refusals_that_need_no_device():
    from charginghub_env_amd import _lib
    L = lib()
    w = np.zeros(tl.WORDS, dtype=np.float64)
    gate = np.zeros(1, dtype=np.int64)
    ps = np.ones(6, dtype=np.float64)
    h, h2 = C.c_void_p(), C.c_void_p()
    m, last = C.c_int64(), C.c_int64()
    args = _lib.ChubPpoUpdateArgs()
    calls = [
        ("create: null env", lambda: L.chub_train_log_create(None, C.byref(h))),
        ("begin: null", lambda: L.chub_train_log_begin_device(None, None)),
        ("record: null", lambda: L.chub_train_log_record_device(None, ptr(ps), ptr(ps), 0, 0.0, None)),
        ("steps: null", lambda: L.chub_train_log_steps_device(None, ptr(ps), ptr(ps), None)),
        ("device: null", lambda: L.chub_train_log_device(None, C.byref(h), C.byref(h2))),
        ("read: null", lambda: L.chub_train_log_read(None, ptr(w))),
        ("fold: null words", lambda: L.chub_train_log_fold(None, ptr(gate), ptr(ps), ptr(ps), 0, 0.0)),
        ("fold: null gate", lambda: L.chub_train_log_fold(ptr(w), None, ptr(ps), ptr(ps), 0, 0.0)),
        ("fold: unknown kl_kind", lambda: L.chub_train_log_fold(ptr(w), ptr(gate), ptr(ps), ptr(ps), 2, 0.0)),
        ("fold: negative kl_kind", lambda: L.chub_train_log_fold(ptr(w), ptr(gate), ptr(ps), ptr(ps), -1, 0.0)),
        ("fold: negative limit", lambda: L.chub_train_log_fold(ptr(w), ptr(gate), ptr(ps), ptr(ps), 0, -0.5)),
        ("fold: NaN limit", lambda: L.chub_train_log_fold(ptr(w), ptr(gate), ptr(ps), ptr(ps), 0, float("nan"))),
        ("set_gate: null", lambda: L.chub_adam_set_gate(None, ptr(gate))),
        ("plan: null out", lambda: L.chub_ppo_update_plan(384, 100, None, C.byref(last))),
        ("plan: n_rows = 0", lambda: L.chub_ppo_update_plan(0, 100, C.byref(m), C.byref(last))),
        ("plan: minibatch_rows = 0", lambda: L.chub_ppo_update_plan(384, 0, C.byref(m), C.byref(last))),
        ("update: null args", lambda: L.chub_ppo_update(None, None)),
        ("update: null objects", lambda: L.chub_ppo_update(C.byref(args), None)),
    ]
    for what, call in calls:
        assert call() == ERR_ARG, what
        assert last_error(), what
    assert L.chub_train_log_destroy(None) == 0
    assert (w == 0).all() and gate[0] == 0


def test_the_wrong_variants_show_on_the_made_sequences():
    """the failure experiment on the CPU twin: which of the made sequences (the ones the GPU test runs through the kernels too) tell a
    wrong log from the restatement.  (c), the gate read by one workgroup only, is a property of the step kernel: its twin is the next
    test, and tests/test_gpu_trainlog.py's gated steps on three chunks and on 83 chunks hold the device to it."""
    shows = {wrong: [name for name, seq in SEQ.items() if not np.array_equal(tl.bits(tl.restate(seq).w), tl.bits(tl.restate(seq, wrong).w))]
             for wrong in tl.WRONG}
    print(shows)
    stopping = sorted(name for name, seq in SEQ.items() if seq["stopped_at"] is not None)
    assert sorted(shows["stop_not_counted"]) == stopping, "(a) every sequence that stops"
    assert sorted(shows["stop_not_sticky"]) == sorted(n for n in stopping if SEQ[n]["after_stop"]), "(b) every sequence with a record after the stop"
    assert shows["gt_limit"] == ["nan"], "(d) the NaN alone"


@pytest.mark.parametrize("net", ["13-33-47", "64-256-224-47"])
def test_a_gate_read_by_workgroup_0_alone_shows_on_both_nets(net):
    """(c) of the failure experiment, on the CPU twin of the gated step: with the gate closed the right step keeps every bit; the wrong one
    keeps workgroup 0's chunks only, so theta, m and v differ wherever another workgroup has a chunk -- two of three chunks of the small
    net, 81 of 83 of the wide one, whose workgroups 0 .. 18 make a second trip"""
    import adam_lib as al
    F, widths = {"13-33-47": (13, [33, 47]), "64-256-224-47": al.ACTOR_NETS["64-256-224-47"]}[net]
    shapes = al.shapes_of(F, widths)
    n = al.n_params(shapes, 2)
    rs = np.random.RandomState(4)
    theta, g = rs.normal(size=n).astype(np.float32), rs.normal(size=n).astype(np.float32)
    hyper = dict(lr=3e-3, max_grad_norm=0.5, weight_decay=0.01)
    right, wrong = al.Adam(n, al.decay_mask(shapes, 2), **hyper), al.Adam(n, al.decay_mask(shapes, 2), **hyper)
    blob = right.blob()
    th_r, st_r = tl.gated_step(right, theta, g, 1)
    th_w, st_w = tl.gated_step(wrong, theta, g, 1, wrong="gate_workgroup_0")
    assert np.array_equal(th_r.view(np.uint32), theta.view(np.uint32)) and right.blob() == blob and list(st_r[[0, 2, 3]]) == [0, 0, 2]
    moved = th_w.view(np.uint32) != theta.view(np.uint32)
    chunks = (n + al.CHUNK - 1) // al.CHUNK
    kept = [c for c in range(chunks) if c % min(chunks, al.MAX_BLOCKS) == 0]
    assert kept == ([0] if chunks == 3 else [0, 64]) and not moved[:1024].any() and moved[1024:2048].mean() > 0.99 and wrong.blob() != blob
    assert list(st_w) == list(st_r), "the stats alone would not show it"
    th_o, st_o = tl.gated_step(al.Adam(n, al.decay_mask(shapes, 2), **hyper), theta, g, 0)
    assert st_o[3] == 0 and (th_o.view(np.uint32) != theta.view(np.uint32)).mean() > 0.99
