"""Weight EMA, the parts that need no GPU: ModelEMA.decay_at, the argument refusals of
ivit_adamw_chunked_ema / ivit_swap_chunked (each before any device call, with a message), the new
flags of the training and evaluation parsers, and the header's declarations. No kernel is launched."""
import ctypes
import inspect
import os

import pytest
import torch

import _lib
from conftest import REPO

LIB = os.path.join(REPO, "visiontransformer-intention-prediction_amd", "libivit_hip.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="libivit_hip.so not built (run __graft_entry__.build())")


def _ema(decay, warmup):
    """A ModelEMA's host side without a device: decay_at reads only these two fields."""
    import optim
    e = optim.ModelEMA.__new__(optim.ModelEMA)
    e.decay, e.warmup = float(decay), bool(warmup)
    return e


def test_decay_at():
    e = _ema(0.9998, True)
    assert e.decay_at(1) == 2.0 / 11.0
    assert [e.decay_at(n) for n in (2, 3)] == [3.0 / 12.0, 4.0 / 13.0]
    # the crossover: (1 + n) / (10 + n) >= 0.9998 first at n = 44990 ((1 + n) >= 0.9998 (10 + n) <=> n >= 44990)
    assert e.decay_at(44989) == 44990.0 / 44999.0 < 0.9998
    assert e.decay_at(44990) == 0.9998 and e.decay_at(10 ** 7) == 0.9998
    # a small decay is never bound by the ramp (2/11 > 0.1), and warmup off is the constant
    assert all(_ema(0.1, True).decay_at(n) == 0.1 for n in (1, 2, 3, 100))
    assert all(_ema(0.9998, False).decay_at(n) == 0.9998 for n in (1, 2, 3, 100))
    h = _ema(0.5, True)  # 0.5: bound at n = 1..7 ((1 + n) / (10 + n) < 1/2 <=> n < 8)
    assert [h.decay_at(n) for n in (1, 7, 8, 9)] == [2.0 / 11.0, 8.0 / 17.0, 0.5, 0.5]


def test_model_ema_rejects_on_the_host():
    import optim
    p = torch.nn.Parameter(torch.zeros(4))
    for bad in (1.0, -0.1, float("nan"), 2.0):
        with pytest.raises(ValueError, match="decay"):
            optim.ModelEMA([p], decay=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        optim.ModelEMA([p], decay=0.9)
    with pytest.raises(ValueError, match="no parameters"):
        optim.ModelEMA([], decay=0.9)
    sig = inspect.signature(optim.ModelEMA.__init__)
    assert sig.parameters["decay"].default == 0.9998 and sig.parameters["warmup"].default is True
    assert list(inspect.signature(optim.FusedAdamW.step_ema).parameters) == ["self", "ema", "closure", "finite", "grad_scale"]
    from trainer import Trainer
    opt = optim.FusedAdamW([p])
    assert Trainer(torch.nn.Linear(2, 2), None, opt, None).ema is None
    with pytest.raises(TypeError, match="ModelEMA"):
        Trainer(torch.nn.Linear(2, 2), None, opt, None, ema=object())
    with pytest.raises(TypeError, match="FusedAdamW"):
        Trainer(torch.nn.Linear(2, 2), None, torch.optim.AdamW([p]), None, ema=_ema(0.9, False))


def test_header_declares_both_symbols():
    protos = _lib.parse_header()
    dll = _lib.lib.load()
    for name in ("ivit_adamw_chunked_ema", "ivit_swap_chunked"):
        assert name in protos and hasattr(dll, name), name
    scaled, ema = protos["ivit_adamw_chunked_scaled"][1], protos["ivit_adamw_chunked_ema"][1]
    # the scaled update's arguments plus (emas, ema_decay, ema_warmup), before the stream
    assert ema == scaled[:-1] + [ctypes.c_void_p, ctypes.c_double, ctypes.c_int] + scaled[-1:]
    assert protos["ivit_swap_chunked"] == (ctypes.c_int, [ctypes.c_long] + [ctypes.c_void_p] * 4 + [ctypes.c_long] +
                                           [ctypes.c_void_p] * 2)


def _buf():
    buf = (ctypes.c_double * 8)()
    return buf, ctypes.addressof(buf)


def test_adamw_ema_refusals():
    dll = _lib.lib.load()
    keep, b = _buf()
    tabs = (b, b, b, b, None, b)
    hyper = (1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0, 1.0)
    call = lambda chunks, nch, steps, emas, decay, warm: dll.ivit_adamw_chunked_ema(
        1, *tabs, chunks, nch, *hyper, None, *steps, None, emas, decay, warm, None)
    for bad in (1.0, -0.1, float("nan"), 1.5):
        assert call(b, 1, (None, None), b, bad, 0) != 0
        assert b"ema_decay must be in [0, 1)" in dll.ivit_last_error(), dll.ivit_last_error()
        assert call(b, 0, (None, None), b, bad, 0) != 0  # an empty launch does not hide a bad decay
    # the ramp needs the device counts
    assert call(b, 1, (None, None), b, 0.9, 1) != 0
    assert b"ema_warmup needs the device step counts" in dll.ivit_last_error()
    assert call(b, 1, (None, None), b + 4, 0.9, 0) != 0
    assert b"misaligned ema table" in dll.ivit_last_error()
    # the checks of the chunked entry
    for chunks, steps, msg in ((None, (None, None), b"bad chunk table"), (b + 4, (None, None), b"misaligned chunk table"),
                               (b, (b, None), b"steps_in / steps_out pair"), (b, (b, b), b"aliases")):
        assert call(chunks, 1, steps, b, 0.9, 0) != 0
        assert msg in dll.ivit_last_error() and b"ivit_adamw_chunked_ema" in dll.ivit_last_error()
    # nothing to do; and a null table is the scaled entry (which does not look at the decay)
    assert call(b, 0, (None, None), b, 0.9, 0) == 0
    assert call(b, 0, (None, None), None, 7.0, 0) == 0
    assert call(None, 1, (None, None), None, 0.9, 0) != 0
    assert b"ivit_adamw_chunked: bad chunk table" in dll.ivit_last_error()
    with pytest.raises(RuntimeError, match="ivit_adamw_chunked_ema failed"):
        _lib.lib.ivit_adamw_chunked_ema(1, *tabs, b, 1, *hyper, None, None, None, None, b, 1.0, 0, None)


def test_swap_refusals():
    dll = _lib.lib.load()
    keep, b = _buf()
    assert dll.ivit_swap_chunked(0, None, None, None, None, 0, None, None) == 0  # nothing to do
    assert dll.ivit_swap_chunked(1, b, b, b, b, 0, None, None) == 0
    for args, msg in (((1, b, b, b, None, 1, None, None), b"bad chunk table"),
                      ((1, b, b, b, b + 4, 1, None, None), b"misaligned chunk table"),
                      ((1, b, b, b, b, 1 << 31, None, None), b"bad chunk table"),
                      ((1, None, b, b, b, 1, None, None), b"null tensor tables"),
                      ((1, b, None, b, b, 1, None, None), b"null tensor tables"),
                      ((1, b, b, None, b, 1, None, None), b"null tensor tables")):
        assert dll.ivit_swap_chunked(*args) != 0
        assert msg in dll.ivit_last_error() and b"ivit_swap_chunked" in dll.ivit_last_error()


def test_flags_parse_with_defaults_off():
    import eval_cnn  # noqa: F401  (shares eval_vit's parser)
    import eval_vit
    import train_cnn
    import train_vit
    for mod in (train_vit, train_cnn):
        a = mod.parse_args([])
        assert a.ema_decay is None and a.ema_no_warmup is False
        a = mod.parse_args(["--ema-decay", "0.999", "--ema-no-warmup"])
        assert a.ema_decay == 0.999 and a.ema_no_warmup is True
    assert eval_vit.parse_args([]).ema is False
    assert eval_vit.parse_args(["--ema"]).ema is True
