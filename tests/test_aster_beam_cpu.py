"""CPU: the ASTER beam-search fixture (tests/golden/aster_beam.npz, from the imported reference) meets the conditions its generator
enforces -- recomputed here from the float64 restatement, which must reproduce the stored reference ids and histories -- and the host-side
refusals of the decode (beam_search, RecognizerBuilder, the four C entry points) hold with no device."""
import ctypes

import numpy as np
import pytest
import torch

from tests.aster_beam_common import (GAP, backtrack_ref, beam_search_ref, beam_state_dict, beam_step_ref, conditions, conditions_hold, fixture,
                                     topk_lower_index)


@pytest.fixture(scope="module")
def g():
    return fixture()


@pytest.fixture(scope="module")
def restated(g):
    """the float64 restatement on the fixture's features, both widths, computed once"""
    eos, C, L = int(g["eos"]), int(g["num_classes"]), int(g["max_len"])
    sd = beam_state_dict(int(g["seed"]), eos, float(g["eos_bias"]))
    feats = torch.tensor(g["feats"])
    with torch.no_grad():
        return {int(B): beam_search_ref(sd, feats, C, L, int(B), eos) for B in g["widths"]}


def test_fixture_shapes(g):
    assert g["feats"].shape == (4, 25, 512) and int(g["max_len"]) == 12 and int(g["num_classes"]) == 97 and int(g["eos"]) == 94
    assert sorted(int(b) for b in g["widths"]) == [3, 5] and float(g["gap"]) == GAP
    for B in (5, 3):
        assert g[f"ids_b{B}"].shape == (4, 12) and g[f"score_hist_b{B}"].shape == (12, 4 * B)


def test_restatement_reproduces_the_reference_ids(g, restated):
    for B, r in restated.items():
        assert torch.equal(r["ids"], torch.tensor(g[f"ids_b{B}"])), (B, r["ids"].tolist(), g[f"ids_b{B}"].tolist())
        assert torch.equal(r["sym"], torch.tensor(g[f"sym_hist_b{B}"]).long()) and torch.equal(r["pred"], torch.tensor(g[f"pred_hist_b{B}"]).long())
        assert torch.equal(r["best_len"], torch.tensor(g[f"best_len_b{B}"]))
        assert (r["score"] - torch.tensor(g[f"score_hist_b{B}"])).abs().max().item() < 1e-9
        assert (r["best_score"] - torch.tensor(g[f"best_score_b{B}"])).abs().max().item() < 1e-9


def test_fixture_meets_its_conditions(g, restated):
    eos, L = int(g["eos"]), int(g["max_len"])
    for B, r in restated.items():
        c = conditions(g[f"score_hist_b{B}"], g[f"sym_hist_b{B}"], g[f"pred_hist_b{B}"], r["gaps"], 4, B, L, eos)      # gaps: recomputed
        print(f"B={B}: min gap {c['min_gap']:.3e}, final gap {c['final_gap']:.3e}, (a) {c['never_eos']} (b) {c['ends_early']} "
              f"(c) {c['wraps']} (d) {c['together']}")
        assert c["finite"] and c["min_gap"] >= GAP and c["final_gap"] >= GAP
        assert torch.equal(c["bt"]["ids"], torch.tensor(g[f"ids_b{B}"]))            # the stored histories backtrack to the stored ids
        assert (r["gaps"] - torch.tensor(g[f"gaps_b{B}"])).abs().max().item() < 1e-9
        if B == 5:
            assert conditions_hold(c)


def test_order_of_equal_values():
    v = torch.tensor([[1.0, 3.0, 3.0, float("nan"), float("-inf"), 3.0]])
    vals, idx = topk_lower_index(v, 6)
    assert idx.tolist() == [[1, 2, 5, 0, 3, 4]] and vals[0, 4].item() == float("-inf")
    st = beam_step_ref(torch.zeros(2, 3, dtype=torch.float64), torch.tensor([0.0, 0.0], dtype=torch.float64), 1, 2, 3, 2)
    assert st["sym"].tolist() == [0, 1] and st["pred"].tolist() == [0, 0]
    bt = backtrack_ref(torch.tensor([[0.5, 0.5]]).double(), torch.tensor([[1, 0]]), torch.tensor([[0, 1]]), 1, 2, 1, 9)
    assert bt["ids"].tolist() == [[1]] and bt["best_len"].tolist() == [1]


def _head():
    from tpgsr_amd.model.recognizer.attention_recognition_head import AttentionRecognitionHead
    return AttentionRecognitionHead(num_classes=97, in_planes=512, sDim=512, attDim=512, max_len_labels=4)


@pytest.mark.parametrize("width", [0, 9, -1, 2.0, "5", None, True])
def test_beam_search_refuses_a_bad_width(width):
    with pytest.raises(ValueError, match="beam_width"):
        _head().beam_search(torch.zeros(1, 25, 512), width, 94)


@pytest.mark.parametrize("eos", ["EOS", 94.0, None, True])
def test_beam_search_refuses_a_non_integer_eos(eos):
    with pytest.raises(ValueError, match="eos"):
        _head().beam_search(torch.zeros(1, 25, 512), 5, eos)


def test_beam_search_refuses_too_many_candidates():
    from tpgsr_amd.model.recognizer.attention_recognition_head import AttentionRecognitionHead
    head = AttentionRecognitionHead(num_classes=200, in_planes=8, sDim=8, attDim=8, max_len_labels=2)
    with pytest.raises(ValueError, match="512"):
        head.beam_search(torch.zeros(1, 3, 8), 3, 1)


def test_recognizer_builder_beam_width_argument():
    from tpgsr_amd.model.recognizer import RecognizerBuilder
    kw = dict(arch="ResNet_ASTER", rec_num_classes=97, max_len_labels=4)
    assert RecognizerBuilder(**kw).beam_width == 0                             # the default stays the greedy decode, string eos and all
    assert RecognizerBuilder(eos=94, beam_width=5, **kw).beam_width == 5
    with pytest.raises(ValueError, match=r'voc\.index\("EOS"\)'):
        RecognizerBuilder(beam_width=5, **kw)                                  # the constructor's default eos is the string "EOS"
    for bad in (9, -1, 2.5, "5"):
        with pytest.raises(ValueError, match="beam_width"):
            RecognizerBuilder(eos=94, beam_width=bad, **kw)


@pytest.fixture(scope="module")
def lib():
    from tpgsr_amd import build
    path = build.build()
    h = ctypes.CDLL(path)
    h.tpgsr_last_error.restype = ctypes.c_char_p
    return h


P = ctypes.c_void_p
I = ctypes.c_int


def _call(lib, name, types, args):
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = ctypes.c_int, list(types) + [P]
    return fn(*args, None), lib.tpgsr_last_error()


A_, B_, C_, D_, E_, F_ = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000      # never dereferenced: every call is refused before a launch


@pytest.mark.parametrize("N,B,C,word", [(1, 0, 97, b"1 .. 8"), (1, 9, 37, b"1 .. 8"), (1, 5, 0, b"512"), (1, 5, 103, b"512"), (1, 8, 65, b"512"),
                                        (0, 5, 97, b"N"), (-3, 5, 97, b"N")])
def test_beam_step_rejects_sizes(lib, N, B, C, word):
    rc, msg = _call(lib, "tpgsr_beam_step", [P, P, I, I, I, I, P, P, P], (A_, B_, N, B, C, 94, C_, D_, E_))
    assert rc == -1 and b"tpgsr_beam_step" in msg and word in msg, msg


def test_beam_step_rejects_null_pointers(lib):
    ptrs = [A_, B_, C_, D_, E_]
    for i in range(5):
        q = list(ptrs)
        q[i] = None
        rc, msg = _call(lib, "tpgsr_beam_step", [P, P, I, I, I, I, P, P, P], (q[0], q[1], 2, 5, 97, 94, q[2], q[3], q[4]))
        assert rc == -1 and b"null" in msg, (i, msg)


@pytest.mark.parametrize("N,B,L,word", [(1, 0, 12, b"1 .. 8"), (1, 9, 12, b"1 .. 8"), (1, 5, 0, b"L"), (0, 5, 12, b"N"), (1 << 30, 8, 12, b"2^31")])
def test_beam_backtrack_rejects_sizes(lib, N, B, L, word):
    rc, msg = _call(lib, "tpgsr_beam_backtrack", [P, P, P, I, I, I, I, P, P, P], (A_, B_, C_, N, B, L, 94, D_, E_, F_))
    assert rc == -1 and b"tpgsr_beam_backtrack" in msg and word in msg, msg


def test_beam_backtrack_rejects_null_pointers(lib):
    ptrs = [A_, B_, C_, D_, E_, F_]
    for i in range(6):
        q = list(ptrs)
        q[i] = None
        rc, msg = _call(lib, "tpgsr_beam_backtrack", [P, P, P, I, I, I, I, P, P, P], (q[0], q[1], q[2], 2, 5, 12, 94, q[3], q[4], q[5]))
        assert rc == -1 and b"null" in msg, (i, msg)


def test_gather_rows_rejects_bad_arguments(lib):
    sig = [P, P, I, I, P]
    for args, word in (((None, B_, 4, 8, C_), b"null"), ((A_, None, 4, 8, C_), b"null"), ((A_, B_, 4, 8, None), b"null"),
                       ((A_, B_, 0, 8, C_), b"at least 1"), ((A_, B_, 4, 0, C_), b"at least 1"), ((A_, B_, 4, 8, A_), b"different")):
        rc, msg = _call(lib, "tpgsr_gather_rows", sig, args)
        assert rc == -1 and b"tpgsr_gather_rows" in msg and word in msg, (args, msg)


def test_attention_rows_rejects_bad_arguments(lib):
    sig = [P, P, P, P, P, I, I, I, I, I, P, P]
    ptrs = [A_, B_, C_, D_, E_, F_, 0x7000]

    def args(p=ptrs, R=10, rps=5, T=25, A=512, D=512):
        return (p[0], p[1], p[2], p[3], p[4], R, rps, T, A, D, p[5], p[6])
    for i in range(7):
        q = list(ptrs)
        q[i] = None
        rc, msg = _call(lib, "tpgsr_aster_attention_rows", sig, args(p=q))
        assert rc == -1 and b"null" in msg, (i, msg)
    for kw, word in ((dict(R=0), b"rows_per_seq"), (dict(rps=0), b"rows_per_seq"), (dict(R=11), b"rows_per_seq"), (dict(T=257), b"256"),
                     (dict(T=0), b"256"), (dict(A=0), b"A"), (dict(D=0), b"D")):
        rc, msg = _call(lib, "tpgsr_aster_attention_rows", sig, args(**kw))
        assert rc == -1 and b"tpgsr_aster_attention_rows" in msg and word in msg, (kw, msg)


def test_beam_entry_points_are_in_the_binding():
    from tpgsr_amd import _lib
    for sym in ("tpgsr_aster_attention_rows", "tpgsr_beam_step", "tpgsr_gather_rows", "tpgsr_beam_backtrack"):
        assert sym in _lib.EXPORTED_SYMBOLS
    assert len(_lib.ABI_STRUCTS) == 13                        # scalar parameters only: no new argument struct


def test_state_dict_layout_is_unchanged():
    from tests.aster_common import layout
    from tpgsr_amd.model.recognizer import RecognizerBuilder
    net = RecognizerBuilder(arch="ResNet_ASTER", rec_num_classes=97, max_len_labels=12, eos=94, beam_width=5)
    assert [(k, list(v.shape)) for k, v in net.state_dict().items()] == [(k, list(s)) for k, s in layout()]
