"""Host side of the CARS session tail's workspace (csrc/cars_session.hip: sess_plan), no GPU: nir_cars_session_workspace_bytes returns the
sum of the plan's slices -- which no longer holds the [R, 4 D] pair-feature matrix, maxout layer 0 forms those rows while it stages its A
operand -- and nir_cars_rank_session accepts exactly that size: one byte less is NIR_ERR_WORKSPACE before anything is enqueued."""
import ctypes as C

import pytest

from context_attentive_ir_amd import lib

ERR_WORKSPACE = -3
SHAPES = [(2, 3, 5, 64, 32), (1, 1, 1, 64, 16), (16, 7, 10, 256, 256), (3, 2, 70, 128, 48)]


def _weights(D, HS):
    w = lib.CarsSessionWeights()
    w.D, w.HS, w.HDEC = D, HS, 64
    w.q_on = w.d_on = w.rank_on = 1
    return w


def _plan_bytes(B, S, N, D, HS, nch=2):
    """sess_plan's slices in floats (ranker on, decoder states wanted), each starting on a 256-byte boundary"""
    R, BS = B * S * N, B * S
    slices = [R * (D // 16), BS * D] + 4 * [(S + 1) * B * HS] + [BS * (nch * HS + nch + 4), BS * (D + nch * HS), BS * D,
              R * 256, R * 128, (S + 1) * B * (HS // 16), S * B * nch * HS, nch * BS * 4 * HS] + 2 * [(S + 1) * B * HS]
    off = 0
    for n in slices:
        off = (off + 255) // 256 * 256 + 4 * n
    return (off + 255) // 256 * 256


@pytest.mark.parametrize("B,S,N,D,HS", SHAPES)
def test_size_query_is_the_plan_without_the_feature_matrix(B, S, N, D, HS):
    L = lib.load()
    w = _weights(D, HS)
    need = L.nir_cars_session_workspace_bytes(B, S, N, C.byref(w))
    assert need == _plan_bytes(B, S, N, D, HS)
    assert need < _plan_bytes(B, S, N, D, HS) + 4 * B * S * N * 4 * D          # the feature matrix alone was 16 R D bytes


@pytest.mark.parametrize("B,S,N,D,HS", SHAPES)
def test_entry_refuses_one_byte_less_than_the_query(B, S, N, D, HS):
    """every pointer the argument checks look at is non-NULL but never dereferenced: the size check comes before the first launch"""
    L = lib.load()
    w = _weights(D, HS)
    fake = C.c_void_p(256)
    w.wrank = w.attn_ut = fake.value
    need = L.nir_cars_session_workspace_bytes(B, S, N, C.byref(w))
    fp = C.cast(fake, C.POINTER(C.c_float))
    ex = lib.CarsSessionOutputs()                       # the query sizes a call that also wants the decoder-side states
    rc = L.nir_cars_rank_session(fp, fp, fp, B, S, N, C.byref(w), fake, need - 1, fp, None, C.byref(ex), None)
    assert rc == ERR_WORKSPACE
    assert ("%d < %d" % (need - 1, need)).encode() in L.nir_last_error_string()
