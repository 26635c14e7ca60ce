"""CPU: the evaluation entries of the C ABI (include/hoisdf.h hoisdf_eval_*, csrc/eval.hip) refuse malformed calls with
HOISDF_ERR_INVALID and a message naming the argument before anything is launched (no GPU here: a launch would fail loudly), their
size queries are host arithmetic, and the Python switch is off by default."""
import ctypes as C
import os

import pytest

from hoisdf_amd import _lib

INVALID = -1
FAKE = C.c_void_p(0x100000)
ENTRIES = ("hoisdf_eval_object", "hoisdf_eval_hand_joints", "hoisdf_eval_mesh", "hoisdf_eval_accum_init", "hoisdf_eval_accum_feed",
           "hoisdf_eval_accum_finish")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def _refused(lib, name, args, word):
    rc = getattr(lib, name)(*args)
    msg = lib.hoisdf_last_error()
    assert rc == INVALID and word in msg, (name, word, rc, msg)


def _each_pointer_alone(lib, name, full, required):
    for i in required:
        args = list(full)
        assert args[i] is FAKE, (name, i)
        args[i] = None
        _refused(lib, name, args, b"null")


def test_entries_are_bound(lib):
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    for name in ("hoisdf_eval_workspace_bytes", "hoisdf_eval_accum_state_bytes"):
        assert name in _lib._OTHER and hasattr(lib, name), name


def test_object_entry_checks_its_arguments(lib):
    #       rot   trans  P   rot_gt trans_gt tpl  T  V    ids   B  adds  mce   oce   mme   used  ws    bytes    stream
    full = [FAKE, FAKE, 40, FAKE, FAKE, FAKE, 4, 300, FAKE, 6, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 1 << 20, None]
    _each_pointer_alone(lib, "hoisdf_eval_object", full, (0, 1, 3, 4, 5, 8, 10, 11, 12, 13, 14, 15))
    for i, word in ((2, b"P=0"), (6, b"T=0"), (7, b"V=0")):
        args = list(full)
        args[i] = 0
        _refused(lib, "hoisdf_eval_object", args, word)
    args = list(full)
    args[7] = -3
    _refused(lib, "hoisdf_eval_object", args, b"V=-3")
    args = list(full)
    args[9] = -1
    _refused(lib, "hoisdf_eval_object", args, b"B=-1")
    args = list(full)
    args[16] = 16                                                                       # a workspace too small for one distance array
    assert lib.hoisdf_eval_object(*args) == -4 and b"workspace_bytes=16" in lib.hoisdf_last_error()
    zero = [None, None, 40, None, None, None, 4, 300, None, 0, None, None, None, None, None, None, 0, None]
    assert lib.hoisdf_eval_object(*zero) == 0                                          # no samples: nothing to do


def test_hand_joint_entry_checks_its_arguments(lib):
    #       pred  gt    B  J   mje   pamje aligned xform dist  dist_al stream
    full = [FAKE, FAKE, 6, 21, FAKE, FAKE, None, None, None, None, None]
    _each_pointer_alone(lib, "hoisdf_eval_hand_joints", full, (0, 1, 4, 5))
    args = list(full)
    args[3] = 0
    _refused(lib, "hoisdf_eval_hand_joints", args, b"J=0")
    args = list(full)
    args[2] = -2
    _refused(lib, "hoisdf_eval_hand_joints", args, b"B=-2")
    assert lib.hoisdf_eval_hand_joints(None, None, 0, 21, None, None, None, None, None, None, None) == 0


def test_mesh_entry_checks_its_arguments(lib):
    #       pred  gt    B  V    th    nt d_raw d_al  fs    fs_al aligned ws   bytes    stream
    full = [FAKE, FAKE, 6, 778, FAKE, 2, FAKE, FAKE, FAKE, FAKE, None, FAKE, 1 << 24, None]
    _each_pointer_alone(lib, "hoisdf_eval_mesh", full, (0, 1, 4, 6, 7, 8, 9, 11))
    for i, bad, word in ((3, 0, b"V=0"), (3, -1, b"V=-1"), (5, 0, b"n_thresh=0"), (5, 17, b"n_thresh=17"), (5, -1, b"n_thresh=-1"),
                         (2, -1, b"B=-1")):
        args = list(full)
        args[i] = bad
        _refused(lib, "hoisdf_eval_mesh", args, word)
    args = list(full)
    args[12] = 4 * 4 * 6 * 778                                                          # the four distance arrays but no room for the aligned mesh
    assert lib.hoisdf_eval_mesh(*args) == -4 and b"workspace_bytes" in lib.hoisdf_last_error()
    assert lib.hoisdf_eval_mesh(None, None, 0, 778, None, 2, None, None, None, None, None, None, 0, None) == 0


def test_accumulator_entries_check_their_arguments(lib):
    _refused(lib, "hoisdf_eval_accum_init", [None, 778, 100, None], b"null")
    _refused(lib, "hoisdf_eval_accum_init", [FAKE, 0, 100, None], b"V=0")
    _refused(lib, "hoisdf_eval_accum_init", [FAKE, 778, 1, None], b"steps=1")
    _refused(lib, "hoisdf_eval_accum_init", [FAKE, 778, 65536, None], b"steps=65536")      # the range feed and finish accept
    #       state dist  B  V    th    steps stream
    full = [FAKE, FAKE, 6, 778, FAKE, 100, None]
    _each_pointer_alone(lib, "hoisdf_eval_accum_feed", full, (0, 1, 4))
    for i, bad, word in ((3, 0, b"V=0"), (5, 1, b"steps=1"), (5, 0, b"steps=0"), (2, -1, b"B=-1")):
        args = list(full)
        args[i] = bad
        _refused(lib, "hoisdf_eval_accum_feed", args, word)
    assert lib.hoisdf_eval_accum_feed(None, None, 0, 778, None, 100, None) == 0         # no samples: nothing to do
    #       state V    th    steps out   stream
    full = [FAKE, 778, FAKE, 100, FAKE, None]
    _each_pointer_alone(lib, "hoisdf_eval_accum_finish", full, (0, 2, 4))
    for i, bad, word in ((1, 0, b"V=0"), (3, 1, b"steps=1")):
        args = list(full)
        args[i] = bad
        _refused(lib, "hoisdf_eval_accum_finish", args, word)


def test_size_queries_are_host_arithmetic(lib):
    ws, st = lib.hoisdf_eval_workspace_bytes, lib.hoisdf_eval_accum_state_bytes
    assert ws(22, 1000) >= 7 * 4 * 22 * 1000                                            # four distance arrays and an aligned mesh
    assert 0 < ws(1, 1) < ws(1, 50) < ws(1, 778) < ws(22, 778) < ws(22, 1000)
    assert ws(0, 778) > 0                                                               # an empty batch still gets a valid allocation
    assert ws(-1, 778) == -1 and ws(22, 0) == -1 and ws(22, -5) == -1
    assert st(778, 100) >= 8 + 8 * 778 + 4 * 100 * 778                                  # a count, a sum per vertex, a count per (threshold, vertex)
    assert 0 < st(1, 2) < st(778, 2) < st(778, 100) < st(1000, 100) < st(1000, 101)
    assert st(778, 100) % 8 == 0 and st(3, 3) % 8 == 0
    assert st(778, 65535) > 0 and st(778, 65536) == -1
    assert st(-1, 100) == -1 and st(778, -1) == -1 and st(778, 1) == -1 and st(0, 100) == -1


def test_switch_is_off_by_default_and_read_from_the_environment(monkeypatch):
    from hoisdf_amd import metrics as M
    from hoisdf_amd import ops
    from hoisdf_amd.config import Config
    monkeypatch.delenv("HOISDF_METRICS", raising=False)
    assert Config().native_metrics is False and not M.native_metrics_enabled(Config())
    c = Config()
    c.native_metrics = True
    assert M.native_metrics_enabled(c)
    monkeypatch.setenv("HOISDF_METRICS", "native")
    assert M.native_metrics_enabled(Config())
    monkeypatch.setenv("HOISDF_METRICS", "torch")
    assert not M.native_metrics_enabled(Config())
    for name in ("eval_object", "eval_hand_joints", "eval_mesh", "eval_accum_init", "eval_accumulate", "eval_accum_finish"):
        assert hasattr(ops, name), name
    for name in ("obj_metrics_native", "eval_hand_joint_native", "fscore_native", "MeshEvalNative", "Evaluator"):
        assert hasattr(M, name), name


def test_native_functions_have_no_cpu_fallback():
    import torch
    from hoisdf_amd import metrics as M
    with pytest.raises(RuntimeError):
        M.eval_hand_joint_native(torch.zeros(2, 21, 3), torch.zeros(2, 21, 3))
