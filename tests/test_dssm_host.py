"""Host-side (no GPU) checks of the DSSM / CDSSM mirrors: construction through the Ranker wrapper, the reference's state-dict layout
(recorded in tests/golden/dssm.npz / cdssm.npz by generate_dssm.py), the criterion, the CDSSM width check and the 5-tap fold of the
CDSSM convolution (fp64, against Conv1d over the reference's 3-row interleave)."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from context_attentive_ir_amd.config import default_args
from context_attentive_ir_amd.detinit import det_state_dict


@pytest.mark.parametrize("kind", ["dssm", "cdssm"])
def test_ranker_constructs_with_reference_state_dict(kind):
    from context_attentive_ir_amd.wrappers import Ranker
    g = load_golden(kind)
    r = Ranker(default_args(kind, src_vocab_size=200))
    sd = r.network.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["sd_keys"]]
    assert [list(v.shape) for v in sd.values()] == json.loads(str(g["sd_shapes"]))
    assert sum(p.numel() for p in r.network.parameters() if p.requires_grad) == int(g["n_params"])
    r.network.load_state_dict(det_state_dict({k: v.shape for k, v in sd.items()}), strict=True)
    ref_arch = json.loads(str(g["arch"]))
    args = default_args(kind)
    assert {k: getattr(args, k) for k in ref_arch} == ref_arch
    assert args.use_char_ngram == 3 and args.src_vocab_size == 30000


def test_criterion_is_softmax_nll():
    from context_attentive_ir_amd import autograd as A
    from context_attentive_ir_amd.wrappers import ranker as R
    assert {"DSSM", "CDSSM"} <= R.NLL_MODELS and not ({"DSSM", "CDSSM"} & R.BCE_MODELS)
    assert callable(A.softmax_nll)


@pytest.mark.parametrize("ql,dl", [(2, 9), (3, 9), (4, 9), (9, 4), (9, 1)])
def test_cdssm_rejects_widths_below_the_window(ql, dl):
    from context_attentive_ir_amd.rankers import CDSSM
    m = CDSSM(default_args("cdssm", src_vocab_size=50, emsize=8, nhid=6, nout=4))
    q = torch.ones(2, ql, dtype=torch.long)
    d = torch.ones(2, 3, dl, dtype=torch.long)
    with pytest.raises(RuntimeError, match="widths >= 5"):
        m(q, None, d, None)


def _interleave_conv(x, conv_w, conv_b, window=3):
    """the reference's cdssm.py:33-41 + Conv1d over the interleave (written here in torch)"""
    L = x.shape[1]
    inter = torch.cat([x[:, i:L - window + 1 + i] for i in range(window)], -1)
    return F.conv1d(inter.transpose(1, 2), conv_w, conv_b).transpose(1, 2)


def test_fold_taps_matches_conv_over_interleave_fp64():
    from context_attentive_ir_amd.rankers.cdssm import fold_taps
    g = torch.Generator().manual_seed(3)
    E, O, R, L = 7, 5, 3, 11
    x = torch.randn(R, L, E, generator=g, dtype=torch.float64)
    w = torch.randn(O, 3 * E, 3, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(O, generator=g, dtype=torch.float64)
    ref = _interleave_conv(x, w, b)                                                    # [R, L-4, O]
    w5 = fold_taps(w)
    assert w5.shape == (O, 5, E)
    rows = torch.cat([x[:, m:m + L - 4] for m in range(5)], 2)                       # [R, L-4, 5E]
    out = rows @ w5.reshape(O, 5 * E).t() + b
    torch.testing.assert_close(out, ref, rtol=0, atol=1e-12)
    # the gradient unfolds as dW[o, i E + e, k] = dW5[o, i + k, e]
    gy = torch.randn(ref.shape, generator=g, dtype=torch.float64)
    (gw_ref,) = torch.autograd.grad((ref * gy).sum(), w)
    w5d = fold_taps(w)
    (gw5,) = torch.autograd.grad((rows @ w5d.reshape(O, 5 * E).t() * gy).sum(), w5d)
    unfolded = torch.stack([torch.cat([gw5[:, i + k] for i in range(3)], 1) for k in range(3)], 2)
    torch.testing.assert_close(unfolded, gw_ref, rtol=0, atol=1e-10)
    (gw,) = torch.autograd.grad((rows @ fold_taps(w).reshape(O, 5 * E).t() * gy).sum(), w)
    torch.testing.assert_close(gw, gw_ref, rtol=0, atol=1e-10)


def test_models_need_the_device():
    from context_attentive_ir_amd.rankers import DSSM
    m = DSSM(default_args("dssm", src_vocab_size=50, emsize=8, nhid=6, nout=4))
    with pytest.raises(RuntimeError, match="ROCm device"):
        m(torch.ones(2, 3, dtype=torch.long), None, torch.ones(2, 3, 4, dtype=torch.long), None)


@pytest.mark.parametrize("kind,emsize,nhid,nout,limit", [
    ("dssm", 513, 300, 128, "emsize 513 unsupported .*<= 512"),
    ("dssm", 300, 300, 257, "nout 257 unsupported .*<= 256"),
    ("dssm", 512, 13825, 128, "nhid 13825 unsupported at emsize 512 .*65536 bytes of LDS"),
    ("cdssm", 1018, 320, 128, "emsize 1018 unsupported .*<= 1017"),
    ("cdssm", 300, 321, 128, "nhid 321 unsupported .*<= 320"),
    ("cdssm", 300, 300, 257, "nout 257 unsupported .*<= 256"),
])
def test_models_reject_sizes_the_eval_kernels_cannot_run(kind, emsize, nhid, nout, limit):
    """The training operators accept any size, the eval kernels do not (csrc/dssm.hip): construction refuses what a later predict() would,
    naming the limit, and the largest admitted sizes still construct."""
    from context_attentive_ir_amd.rankers import CDSSM, DSSM
    from context_attentive_ir_amd.wrappers import Ranker
    cls = DSSM if kind == "dssm" else CDSSM
    with pytest.raises(ValueError, match=limit):
        cls(default_args(kind, src_vocab_size=20, emsize=emsize, nhid=nhid, nout=nout))
    with pytest.raises(ValueError, match=limit):
        Ranker(default_args(kind, src_vocab_size=20, emsize=emsize, nhid=nhid, nout=nout))
    for bad in (dict(emsize=0), dict(nhid=0), dict(nout=0)):
        with pytest.raises(ValueError, match="unsupported"):
            cls(default_args(kind, src_vocab_size=20, **dict(dict(emsize=8, nhid=6, nout=4), **bad)))
    biggest = dict(emsize=512, nhid=13824, nout=256) if kind == "dssm" else dict(emsize=1017, nhid=320, nout=256)
    cls(default_args(kind, src_vocab_size=4, **biggest))
