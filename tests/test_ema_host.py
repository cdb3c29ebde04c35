"""Host-side checks of the EMA weight averaging (csrc/ema.hip, optim.AdamW(ema_decay=, ema_warmup=),
train_stage, the CLIs) that need no GPU:

* both C-ABI functions are bound and exported, and their argument contract holds: on a GPU-less host
  a call rejected by validation returns PIS_ERR_ARG (-1) with the function's name in the message, a
  call that passes it reaches the launch (PIS_ERR_LAUNCH, -2), and n == 0 is PIS_OK. Pointers are
  never dereferenced on the host, so made-up addresses serve.
* optim.AdamW refuses an ema_decay outside (0, 1), ema_weight(k) gives the hand-computed weights,
  and the EMA methods raise with EMA off.
* train_stage validates inside optimizer.averaged_weights() every epoch, and only when the
  optimizer has ema_decay set.
* both CLIs take --ema-decay and --no-ema-warmup.
"""
import contextlib
import importlib

import pytest
import torch

from physics_informed_image_segmentation_amd import AdamW, _hip
from test_small_kernels_host import A, B_, C_, D_, E_, OFF, PIS_ERR_ARG, PIS_ERR_LAUNCH, PIS_OK, WS
from test_step_loop_host import _Crit, _Loader, _Net

tr = importlib.import_module("physics_informed_image_segmentation_amd.train")  # the module, not train()

ORDER = {
    "pis_adamw_step_ema": ["p", "g", "m", "v", "ema", "n", "lr", "beta1", "beta2", "eps", "weight_decay",
                           "step_size", "bc2_sqrt", "grad_scale", "ema_weight", "record", "stream"],
    "pis_arena_exchange": ["a", "b", "n", "stream"],
}
GOOD = {
    "pis_adamw_step_ema": dict(p=A, g=B_, m=C_, v=D_, ema=E_, n=8, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
                               weight_decay=1e-2, step_size=1e-3, bc2_sqrt=1.0, grad_scale=1.0, ema_weight=0.1,
                               record=0, stream=0),
    "pis_arena_exchange": dict(a=A, b=B_, n=8, stream=0),
}


def _invoke(lib, fn, changes):
    a = dict(GOOD[fn], **changes)
    return getattr(lib, fn)(*[a[k] for k in ORDER[fn]])


def _case(fn, **changes):
    return pytest.param(fn, changes, id=fn[4:] + "-" + "-".join(f"{k}={v}" for k, v in changes.items()))


BAD_CALLS = [
    _case("pis_adamw_step_ema", p=0), _case("pis_adamw_step_ema", g=0), _case("pis_adamw_step_ema", m=0),
    _case("pis_adamw_step_ema", v=0), _case("pis_adamw_step_ema", ema=0), _case("pis_adamw_step_ema", n=-1),
    _case("pis_adamw_step_ema", p=A + OFF), _case("pis_adamw_step_ema", g=B_ + OFF),
    _case("pis_adamw_step_ema", m=C_ + OFF), _case("pis_adamw_step_ema", v=D_ + OFF),
    _case("pis_adamw_step_ema", ema=E_ + OFF), _case("pis_adamw_step_ema", record=WS + OFF),
    _case("pis_adamw_step_ema", ema_weight=-0.001), _case("pis_adamw_step_ema", ema_weight=1.001),
    _case("pis_adamw_step_ema", ema_weight=float("nan")), _case("pis_adamw_step_ema", ema_weight=float("inf")),
    # a bad argument is refused before n == 0 can answer PIS_OK
    _case("pis_adamw_step_ema", n=0, ema_weight=2.0), _case("pis_adamw_step_ema", n=0, ema=0),
    _case("pis_arena_exchange", a=0), _case("pis_arena_exchange", b=0), _case("pis_arena_exchange", n=-1),
    _case("pis_arena_exchange", a=A + OFF), _case("pis_arena_exchange", b=B_ + OFF),
    _case("pis_arena_exchange", b=A),                   # the same range
    _case("pis_arena_exchange", b=A + 16, n=8),         # b starts inside a
    _case("pis_arena_exchange", a=B_ + 16, n=5),        # a starts inside b
    _case("pis_arena_exchange", b=A + 16, n=5),         # 20 bytes against a distance of 16
    _case("pis_arena_exchange", a=A, b=A, n=0),
]

LEGAL_CALLS = [
    _case("pis_adamw_step_ema"), _case("pis_adamw_step_ema", record=WS), _case("pis_adamw_step_ema", record=WS + 8),
    _case("pis_adamw_step_ema", ema_weight=0.0), _case("pis_adamw_step_ema", ema_weight=1.0),
    _case("pis_adamw_step_ema", n=3),
    _case("pis_arena_exchange"), _case("pis_arena_exchange", n=3),
    _case("pis_arena_exchange", b=A + 32, n=8),         # adjacent ranges do not overlap
    _case("pis_arena_exchange", b=A + 16, n=4),
]


@pytest.fixture(scope="module")
def hostlib():
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: a call that slips through validation would launch with these arguments")
    return _hip.lib()


def test_symbols_bound_and_exported():
    lib = _hip.lib()
    for name in ORDER:
        assert name in _hip.exported_symbols()
        assert getattr(lib, name).restype is _hip.c_int
        assert len(getattr(lib, name).argtypes) == len(ORDER[name])
    assert lib.pis_version() == 1


@pytest.mark.parametrize("fn,changes", BAD_CALLS)
def test_bad_call_is_rejected_before_the_launch(hostlib, fn, changes):
    rc = _invoke(hostlib, fn, changes)
    msg = hostlib.pis_last_error() or b""
    assert rc == PIS_ERR_ARG, (rc, msg)
    assert fn.encode() in msg, msg


@pytest.mark.parametrize("fn,changes", LEGAL_CALLS)
def test_legal_call_reaches_the_launch(hostlib, fn, changes):
    rc = _invoke(hostlib, fn, changes)
    assert rc == PIS_ERR_LAUNCH, (rc, hostlib.pis_last_error())


@pytest.mark.parametrize("fn", list(ORDER))
def test_of_nothing_is_a_no_op(hostlib, fn):
    assert _invoke(hostlib, fn, dict(n=0)) == PIS_OK


def test_error_messages_name_the_argument(hostlib):
    for changes, word in ((dict(ema_weight=1.5), b"ema_weight"), (dict(ema=E_ + OFF), b"16-byte"),
                          (dict(record=WS + OFF), b"8-byte")):
        assert _invoke(hostlib, "pis_adamw_step_ema", changes) == PIS_ERR_ARG
        assert word in hostlib.pis_last_error()
    assert _invoke(hostlib, "pis_arena_exchange", dict(b=A)) == PIS_ERR_ARG
    assert b"overlap" in hostlib.pis_last_error()


# ---------------------------------------------------------------------------------------------
# optim.AdamW
# ---------------------------------------------------------------------------------------------
def _param():
    return [torch.nn.Parameter(torch.zeros(4))]


@pytest.mark.parametrize("bad", [0, 1, -0.1, float("nan"), 0.0, 1.0, 1.5])
def test_adamw_rejects_bad_ema_decay(bad):
    with pytest.raises(ValueError, match="ema_decay"):
        AdamW(_param(), ema_decay=bad)


def test_adamw_keeps_the_options_as_attributes():
    plain = AdamW(_param())
    assert plain.ema_decay is None and plain.ema_warmup is True
    opt = AdamW(_param(), ema_decay=0.99, ema_warmup=False)
    assert opt.ema_decay == 0.99 and opt.ema_warmup is False
    assert set(opt.param_groups[0]) == set(plain.param_groups[0])  # not in the groups, as max_grad_norm
    assert "ema_decay" not in opt.param_groups[0]


def test_ema_weight_by_hand():
    """w_k = 1 - min(d, (1 + k) / (10 + k)): k = 1 gives 1 - 2/11 = 9/11, k = 2 gives 9/12; d = 0.999
    takes over where (1 + k) / (10 + k) >= 0.999, i.e. k >= 8990; without warm-up it is 1 - d always."""
    opt = AdamW(_param(), ema_decay=0.999)
    assert opt.ema_weight(1) == 1.0 - 2.0 / 11.0
    assert opt.ema_weight(1) == pytest.approx(9.0 / 11.0, rel=1e-15)
    assert opt.ema_weight(2) == 1.0 - 3.0 / 12.0 == 0.75
    assert opt.ema_weight(8989) == 1.0 - 8990.0 / 8999.0 > 1.0 - 0.999
    assert opt.ema_weight(8991) == 1.0 - 0.999
    assert opt.ema_weight(10 ** 6) == 1.0 - 0.999
    small = AdamW(_param(), ema_decay=0.1)  # below the warm-up's first value 2/11
    assert small.ema_weight(1) == 1.0 - 0.1
    cold = AdamW(_param(), ema_decay=0.999, ema_warmup=False)
    assert cold.ema_weight(1) == cold.ema_weight(50) == 1.0 - 0.999
    assert isinstance(opt.ema_weight(3), float)


def test_ema_methods_raise_when_off():
    opt = AdamW(_param())
    with pytest.raises(RuntimeError, match="ema_decay"):
        opt.ema_arena()
    with pytest.raises(RuntimeError, match="ema_decay"):
        with opt.averaged_weights():
            pass
    with pytest.raises(RuntimeError, match="ema_decay"):
        opt.ema_state_dict(torch.nn.Linear(1, 1))
    with pytest.raises(RuntimeError, match="ema_decay"):
        opt.ema_weight(1)
    assert "ema" not in opt.state_dict()["state"].get(0, {})


# ---------------------------------------------------------------------------------------------
# train_stage
# ---------------------------------------------------------------------------------------------
class _StubOpt(torch.optim.SGD):
    """Optimizer stand-in that records the exchanges; `log` is shared with the validation loader."""

    def __init__(self, params, log, ema):
        super().__init__(params, lr=0.0)
        self.log = log
        if ema:
            self.ema_decay = 0.9

    @contextlib.contextmanager
    def averaged_weights(self):
        self.log.append("exchange")
        try:
            yield self
        finally:
            self.log.append("exchange")


class _ValLoader(_Loader):
    def __init__(self, log):
        super().__init__()
        self.log = log

    def __iter__(self):
        self.log.append("validate")
        return super().__iter__()


@pytest.mark.parametrize("ema", [True, False])
def test_train_stage_validates_inside_the_exchange(tmp_path, ema):
    log = []
    net, crit = _Net(), _Crit()
    opt = _StubOpt(net.parameters(), log, ema)
    best, ep, hist = tr.train_stage(net, _Loader(), _ValLoader(log), crit, opt, torch.device("cpu"), num_epochs=3,
                                    stage_name="t", verbose=False, csv_path=tmp_path / "m.csv")
    assert len(hist) == 3
    assert log == (["exchange", "validate", "exchange"] if ema else ["validate"]) * 3
    assert set(hist[0]) == set(tr.CSV_FIELDS)
    assert (tmp_path / "m.csv").read_text().splitlines()[0].split(",") == tr.CSV_FIELDS


def test_train_stage_without_the_attribute_is_untouched(tmp_path):
    """torch's own SGD has neither ema_decay nor averaged_weights: today's path."""
    net = _Net()
    opt = torch.optim.SGD(net.parameters(), lr=0.0)
    assert not hasattr(opt, "ema_decay")
    _, _, hist = tr.train_stage(net, _Loader(), _Loader(), _Crit(), opt, torch.device("cpu"), num_epochs=1,
                                stage_name="t", verbose=False)
    assert len(hist) == 1


def test_train_signature_has_the_arguments():
    import inspect
    sig = inspect.signature(tr.train)
    assert sig.parameters["ema_decay"].default is None and sig.parameters["ema_warmup"].default is True


# ---------------------------------------------------------------------------------------------
# CLIs
# ---------------------------------------------------------------------------------------------
def test_cli_flags():
    import main
    import run_ablation
    a = main.parse_args([])
    assert a.ema_decay is None and a.no_ema_warmup is False
    a = main.parse_args(["--ema-decay", "0.999", "--no-ema-warmup"])
    assert a.ema_decay == 0.999 and a.no_ema_warmup is True
    a = run_ablation.parse_args(["--ablation", "R1"])
    assert a.ema_decay is None and a.no_ema_warmup is False
    a = run_ablation.parse_args(["--ablation", "R1", "--ema-decay", "0.9", "--no-ema-warmup"])
    assert a.ema_decay == 0.9 and a.no_ema_warmup is True
    for mod in (main, run_ablation):
        pre = ["--ablation", "R1"] if mod is run_ablation else []
        for bad in ("0", "1", "-0.1", "nan", "x"):
            with pytest.raises(SystemExit):
                mod.parse_args(pre + ["--ema-decay", bad])
