"""not-gpu: the REFERENCE's own classes as seen by THIS engine, held to what the reference does as recorded data.

tests/golden/ref_qmodule.json and ref_from_linear.npz were produced by RUNNING the reference's `awq.quantize.qmodule` and
tinychat/modules/fused_mlp.py (oracle/gen_ref_qmodule.py).  `llm_awq_amd.qmodule` is compared with them member by member: constructor
signature, attributes, registered buffers (names, shapes, dtypes), state_dict entries in both directions, `from_linear` buffers bit for
bit, `extra_repr`, and the engine calls the reference's forward() makes (qmodule.py:206-220), replayed against the MI355X build that
`install_as_awq_inference_engine()` puts under the module name the reference imports (awq/quantize/qmodule.py:4,
tinychat/modules/fused_mlp.py:8)."""
import inspect
import json
import os

import pytest
import torch

from tests.conftest import GOLDEN, as_t

DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16}


@pytest.fixture(scope="module")
def ref_qmodule():
    import llm_awq_amd
    eng = llm_awq_amd.install_as_awq_inference_engine()
    import awq_inference_engine
    assert awq_inference_engine is eng, "`import awq_inference_engine` does not bind the MI355X engine"
    with open(os.path.join(GOLDEN, "ref_qmodule.json")) as f:
        return json.load(f), eng


def _entries(tensors):
    return [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in tensors.items()]


CASES = [(4, 128, 768, 768, True, torch.float16), (4, 128, 4096, 6144, False, torch.bfloat16), (4, 128, 11008, 4096, False, torch.float16),
         (4, -1, 256, 64, True, torch.float16)]


@pytest.mark.parametrize("w_bit,group,K,N,bias,dtype", CASES)
def test_ctor_attributes_buffers_state_dict(ref_qmodule, w_bit, group, K, N, bias, dtype):
    rec, _eng = ref_qmodule
    from llm_awq_amd import qmodule as MQ
    r = rec["cases"][f"{w_bit}-{group}-{K}-{N}-{bias}-{str(dtype).replace('torch.', '')}"]
    assert rec["init_params"] == list(inspect.signature(MQ.WQLinear.__init__).parameters)
    assert rec["from_linear_params"] == list(inspect.signature(MQ.WQLinear.from_linear).parameters)
    m = MQ.WQLinear(w_bit, group, K, N, bias, "cpu", dtype=dtype)
    for a, v in r["attributes"].items():
        assert getattr(m, a) == v, a
    assert _entries(dict(m.named_buffers())) == r["buffers"]
    assert r["bias_is_none"] == (m.bias is None)
    assert m.extra_repr() == r["extra_repr"]
    # state dicts are interchangeable in both directions (the v2 checkpoint contract): ours loads one shaped as the reference's, and
    # saves exactly the reference's entries (names, shapes, dtypes, in order)
    sd = {k: torch.randint(-100, 100, shape).to(DTYPES.get(dt, getattr(torch, dt))) for k, shape, dt in r["state_dict"]}
    m.load_state_dict(sd)
    assert _entries(m.state_dict()) == r["state_dict"]
    for k, v in sd.items():
        assert torch.equal(m.state_dict()[k], v)
    for fn in ("pack_intweight", "calculate_zeros_width", "make_divisible", "ScaledActivation"):
        assert hasattr(MQ, fn) and fn in rec["helpers"]
    assert r["w_bit_2_raises"] == "NotImplementedError"
    with pytest.raises(NotImplementedError):
        MQ.WQLinear(2, 128, K, N, bias, "cpu")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_from_linear_buffers_bit_for_bit(ref_qmodule, dtype, golden):
    from llm_awq_amd import qmodule as MQ
    g = golden("ref_from_linear.npz")
    name = "f16" if dtype == torch.float16 else "bf16"
    fake, s, z = (as_t(g[f"{name}_{k}"], dtype) for k in ("weight", "s", "z"))
    N, K = fake.shape
    lin = torch.nn.Linear(K, N, bias=True, dtype=dtype)
    with torch.no_grad():
        lin.weight.data = fake.clone()
        lin.bias.data = as_t(g[f"{name}_bias_in"], dtype).clone()
    m = MQ.WQLinear.from_linear(lin, 4, 128, False, s.clone(), z.clone())
    for k in ("qweight", "scales", "scaled_zeros", "bias"):
        ref = g[f"{name}_{k}"]
        assert torch.equal(getattr(m, k).detach(), as_t(ref, getattr(m, k).dtype) if k != "qweight" else torch.from_numpy(ref)), k


def test_entry_points_take_the_calls_the_reference_forward_makes(ref_qmodule):
    """qmodule.py:206-220: gemv_forward_cuda_new(x, qweight, scales, scaled_zeros, M, N, K, group_size) for fewer than 8 rows, else
    gemm_forward_cuda_new(x, qweight, scales, scaled_zeros); tinychat/modules/fused_mlp.py:48-77 makes the same two calls.  Here (no GPU):
    the bound functions exist under those names with that arity, and the very calls the reference's forward made (recorded for 1, 7, 8
    and 33 rows) reject CPU tensors loudly instead of computing anything."""
    rec, eng = ref_qmodule
    from llm_awq_amd import qmodule as MQ
    doc_v, doc_m = eng.gemv_forward_cuda_new.__doc__, eng.gemm_forward_cuda_new.__doc__
    sig_v, sig_m = doc_v.split("->")[0], doc_m.split("->")[0]
    assert sig_v.count("torch.Tensor") == 4 and sig_v.count("SupportsInt") == 4 and sig_v.count("arg") == 8   # 4 tensors + m, n, k, group_size
    assert sig_m.count("torch.Tensor") == 4 and sig_m.count("arg") == 4
    w_bit, group, K, N, bias, dt = rec["forward_calls"]["module"]
    m = MQ.WQLinear(w_bit, group, K, N, bias, "cpu", dtype=DTYPES[dt])
    calls = rec["forward_calls"]["calls"]
    assert sorted(int(r) for r in calls) == [1, 7, 8, 33]
    for rows, call in calls.items():  # both branches of the reference's dispatch reach this engine and are refused on CPU tensors
        assert call["fn"] == ("gemv_forward_cuda_new" if int(rows) < 8 else "gemm_forward_cuda_new")
        x = torch.zeros(int(rows), K, dtype=DTYPES[dt])
        args = [x if a == "x" else getattr(m, a) if isinstance(a, str) else a for a in call["args"]]
        with pytest.raises((RuntimeError, ValueError, TypeError)):
            getattr(eng, call["fn"])(*args)


def test_reference_quant_llama_mlp_binds_this_engine(ref_qmodule):
    """tinychat/modules/fused_mlp.py:8 imports awq_inference_engine at module import: with the MI355X build installed under that name the
    reference's QuantLlamaMLP class constructs from WQLinear modules; llm_awq_amd.fused_mlp.QuantLlamaMLP built from this repository's
    WQLinear modules registers the same buffer names and attributes as the reference's did on the same shapes."""
    rec, _eng = ref_qmodule
    from llm_awq_amd.fused_mlp import QuantLlamaMLP
    from llm_awq_amd.qmodule import WQLinear
    r = rec["quant_llama_mlp"]
    mk = lambda k, n: WQLinear(4, 128, k, n, False, "cpu", dtype=torch.float16)  # noqa: E731
    ours = QuantLlamaMLP(*(mk(k, n) for k, n in r["shapes"]))
    assert sorted(dict(ours.named_buffers())) == r["buffer_names"]
    for a, v in r["attributes"].items():
        assert getattr(ours, a) == v, a
