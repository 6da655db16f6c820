"""Host-side pieces of ``orv_amd/stages.py`` (no GPU): the multiview row index and the shape record of a forward."""
import numpy as np
import pytest
import torch

from orv_amd import stages
from orv_amd.cogvideox_control import FrozenConfig


@pytest.mark.parametrize("b,v,f,Nt,P", [(2, 3, 2, 3, 4), (1, 2, 1, 0, 6)])
def test_mv_index_equals_the_rearranged_row_numbers(b, v, f, Nt, P):
    """'(b v) (f s) -> (b f) (v s)' on the video rows, '(b v) n -> (b f) (v n)' on the text rows, built from the row numbers themselves."""
    S = Nt + f * P
    rows = np.arange(b * v * S).reshape(b, v, S)
    txt = np.broadcast_to(rows[:, None, :, :Nt], (b, f, v, Nt)).reshape(b, f, v * Nt)
    vid = rows[:, :, Nt:].reshape(b, v, f, P).transpose(0, 2, 1, 3).reshape(b, f, v * P)
    want = np.concatenate([txt, vid], axis=-1).reshape(-1)
    got = stages.mv_index(b, v, f, Nt, P, S, torch.device("cpu"))
    assert got.dtype == torch.int32 and got.shape == (b * f * v * (Nt + P),)
    assert np.array_equal(got.numpy(), want)
    lay = stages.mv_layout(b, v, f, Nt, P, S, torch.device("cpu"))
    assert torch.equal(lay["idx"], got)
    assert (lay["Sm"], lay["R"], lay["s_pad"]) == (v * (Nt + P), b * f * v * (Nt + P), -(-v * (Nt + P) // 64) * 64)


def _config(**kw):
    return FrozenConfig(dict(patch_size=2, patch_size_t=None, num_attention_heads=2, attention_head_dim=64, time_embed_dim=32,
                             modulate_encoder_hidden_states=True), **kw)


def test_shape_record_folds_the_views_into_the_batch():
    sh = stages.shapes(torch.empty(2, 9, 16, 8, 12), torch.empty(2, 5, 64), 3, _config())
    assert (sh.B, sh.b0, sh.nv, sh.T, sh.Tq, sh.P, sh.Nv, sh.Nt, sh.S, sh.M) == (6, 2, 3, 3, 3, 24, 72, 5, 77, 462)
    assert (sh.C, sh.Hh, sh.Ww, sh.p, sh.pt, sh.D, sh.heads, sh.E, sh.mod_text) == (16, 8, 12, 2, None, 128, 2, 32, True)
    assert (sh.Ta, sh.G, sh.per_group) == (None, None, None)            # known after the action stage


def test_shape_record_with_temporal_patches_and_unmodulated_text():
    sh = stages.shapes(torch.empty(1, 4, 16, 8, 12), torch.empty(1, 5, 64), 1, _config(patch_size_t=2, modulate_encoder_hidden_states=False))
    assert (sh.B, sh.b0, sh.T, sh.Tq, sh.P, sh.Nv, sh.Nt, sh.S, sh.M, sh.pt) == (1, 1, 4, 2, 24, 48, 0, 48, 48, 2)
