"""The operand checks pointer_forced, pointer_sample and pointer_constrained share (ops._step_operands): one bad operand per case,
the ValueError text each op raised before the checks were one helper (literals, recorded from that commit), raised before anything
is launched; and one good call per op with rows and stats.  What the ops compute is checked in test_forced.py / test_sample.py /
test_constrain.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, S, E, SPG, NTOK = 3, 5, 32, 2, 4      # two wireframes: rows 0, 1 and row 2


def _good():
    dev = "cuda"
    return dict(logits=torch.zeros(B, S, device=dev), seqs_per_group=SPG, mask=torch.zeros(2, S, dtype=torch.uint8, device=dev),
                kv_len=torch.full((2,), S, dtype=torch.int32, device=dev), memory=torch.ones(2, S, E, device=dev))


def _call(op, kw):
    from faceformer_amd.hip import ops
    dev = kw["logits"].device
    i32 = lambda fill: torch.full((B,), fill, dtype=torch.int32, device=dev)
    if op == "forced":
        return ops.pointer_forced(kw.pop("logits"), i32(0), **kw)
    if op == "sample":
        return ops.pointer_sample(kw.pop("logits"), torch.full((B,), 0.5, device=dev), **kw)
    return ops.pointer_constrained(kw.pop("logits"), i32(0), i32(-1), i32(-1), torch.zeros(B, 1, dtype=torch.int32, device=dev), 1, NTOK, **kw)


COVER = "%s must be contiguous and cover 2 wireframes of 5 keys"
MEMORY = "memory must be a contiguous [>= 2, 5, E] tensor"
UNIT = "logits must be a 2-D tensor with unit inner stride"
CASES = {
    "3-D logits": (lambda d: dict(logits=torch.zeros(B, 1, S, device=d)), UNIT),
    "logits with inner stride 2": (lambda d: dict(logits=torch.zeros(B, 2 * S, device=d)[:, ::2]), UNIT),
    "seqs_per_group = 0": (lambda d: dict(seqs_per_group=0), "seqs_per_group must be positive"),
    "mask [1, 5]": (lambda d: dict(mask=torch.zeros(1, S, dtype=torch.uint8, device=d)), COVER % "mask"),
    "mask [2, 4]": (lambda d: dict(mask=torch.zeros(2, S - 1, dtype=torch.uint8, device=d)), COVER % "mask"),
    "non-contiguous mask": (lambda d: dict(mask=torch.zeros(2, 2 * S, dtype=torch.uint8, device=d)[:, ::2]), COVER % "mask"),
    "kv_len [1]": (lambda d: dict(kv_len=torch.full((1,), S, dtype=torch.int32, device=d)), COVER % "kv_len"),
    "memory [1, 5, 32]": (lambda d: dict(memory=torch.ones(1, S, E, device=d)), MEMORY),
    "memory [2, 4, 32]": (lambda d: dict(memory=torch.ones(2, S - 1, E, device=d)), MEMORY),
    "want_rows without memory": (lambda d: dict(memory=None, want_rows=True), "rows / stats need memory"),
    "want_stats with E = 16": (lambda d: dict(memory=torch.ones(2, S, 16, device=d), want_stats=True), "stats need E % 32 == 0"),
}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("op", ["forced", "sample", "constrained"])
def test_one_bad_operand_raises_todays_text_before_any_launch(op, case, hip_lib, monkeypatch):
    from faceformer_amd.hip import lib
    change, text = CASES[case]
    kw = dict(_good(), **change("cuda"))
    monkeypatch.setattr(lib, "load", lambda: (_ for _ in ()).throw(AssertionError("library touched")))
    with pytest.raises(ValueError) as e:
        _call(op, kw)
    assert str(e.value) == text


@pytest.mark.parametrize("op", ["forced", "sample", "constrained"])
def test_a_good_call_returns_rows_and_stats_on_the_logits_device(op, hip_lib):
    kw = _good()
    dev = kw["logits"].device
    out = _call(op, dict(kw, want_rows=True, want_stats=True))
    torch.cuda.synchronize()
    assert tuple(out["rows"].shape) == (B, E) and tuple(out["stats"].shape) == (B, E // 32, 2)
    assert out["rows"].device == dev and out["stats"].device == dev
    assert list(out)[-2:] == ["rows", "stats"]
