"""Generate tests/golden/ref_qmodule.json and tests/golden/ref_from_linear.npz by RUNNING THE REFERENCE'S OWN PYTHON (CPU) --
authoring-time only, like oracle/gen_golden.py.

Usage (AWQ_REFERENCE names a checkout of the reference):
    AWQ_REFERENCE=<reference checkout> python oracle/gen_ref_qmodule.py

What tests/test_reference_dropin.py holds this repository's WQLinear / QuantLlamaMLP to, as data:
  * awq/quantize/qmodule.py WQLinear: constructor and from_linear parameter names, attributes, registered buffers (names, shapes,
    dtypes), state_dict entries, extra_repr, the module-level helpers, the exception of an unsupported w_bit (CASES below)
  * WQLinear.from_linear buffers for a seeded input (inputs and outputs in ref_from_linear.npz)
  * WQLinear.forward: the engine calls it makes for 1, 7, 8 and 33 rows (recorded through a stand-in awq_inference_engine)
  * tinychat/modules/fused_mlp.py QuantLlamaMLP: buffer names and attributes
bf16 tensors are stored as their int16 bit patterns (numpy has no bf16).
"""
import importlib.util
import inspect
import json
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("AWQ_REFERENCE")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")

# (w_bit, group_size, in_features, out_features, bias, dtype): the parametrisation of test_ctor_attributes_buffers_state_dict
CASES = [(4, 128, 768, 768, True, torch.float16), (4, 128, 4096, 6144, False, torch.bfloat16), (4, 128, 11008, 4096, False, torch.float16),
         (4, -1, 256, 64, True, torch.float16)]
FORWARD_ROWS = (1, 7, 8, 33)
HELPERS = ("pack_intweight", "calculate_zeros_width", "make_divisible", "ScaledActivation")


def case_key(w_bit, group, K, N, bias, dtype):
    return f"{w_bit}-{group}-{K}-{N}-{bias}-{str(dtype).replace('torch.', '')}"


def bits(t: torch.Tensor) -> np.ndarray:
    if t.dtype in (torch.float16, torch.bfloat16):
        return t.contiguous().view(torch.int16).numpy()
    return t.contiguous().numpy()


def entries(tensors):
    return [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in tensors.items()]


def main():
    if not REF or not os.path.isdir(os.path.join(REF, "awq", "quantize")):
        sys.exit("AWQ_REFERENCE must name a checkout of the reference")
    calls = []

    def recorder(fn):
        def call(*args):
            calls.append((fn, args))
            x = args[0]
            return torch.zeros(x.numel() // x.shape[-1], args[1].shape[0] * 4 if fn == "gemm_forward_cuda_new" else args[5], dtype=x.dtype)
        return call

    stand_in = types.ModuleType("awq_inference_engine")
    stand_in.gemv_forward_cuda_new = recorder("gemv_forward_cuda_new")
    stand_in.gemm_forward_cuda_new = recorder("gemm_forward_cuda_new")
    sys.modules["awq_inference_engine"] = stand_in
    sys.path.insert(0, REF)
    import awq.quantize.qmodule as RQ
    from awq.quantize.quantizer import pseudo_quantize_tensor

    rec = {"init_params": list(inspect.signature(RQ.WQLinear.__init__).parameters),
           "from_linear_params": list(inspect.signature(RQ.WQLinear.from_linear).parameters),
           "helpers": [h for h in HELPERS if hasattr(RQ, h)], "cases": {}}
    for (w_bit, group, K, N, bias, dtype) in CASES:
        r = RQ.WQLinear(w_bit, group, K, N, bias, "cpu", dtype=dtype)
        try:
            RQ.WQLinear(2, 128, K, N, bias, "cpu")
            w2 = None
        except Exception as e:  # noqa: BLE001
            w2 = type(e).__name__
        rec["cases"][case_key(w_bit, group, K, N, bias, dtype)] = {
            "attributes": {a: getattr(r, a) for a in ("in_features", "out_features", "w_bit", "group_size", "split_k_iters", "interleave")},
            "buffers": entries(dict(r.named_buffers())), "bias_is_none": r.bias is None, "extra_repr": r.extra_repr(),
            "state_dict": entries(r.state_dict()), "w_bit_2_raises": w2}

    # forward: which entry point, with which arguments, for each row count (tensors named by the module buffer they are)
    r = RQ.WQLinear(4, 128, 256, 64, False, "cpu", dtype=torch.float16)
    names = {id(r.qweight): "qweight", id(r.scales): "scales", id(r.scaled_zeros): "scaled_zeros"}
    rec["forward_calls"] = {"module": [4, 128, 256, 64, False, "float16"], "calls": {}}
    for rows in FORWARD_ROWS:
        calls.clear()
        x = torch.zeros(rows, 256, dtype=torch.float16)
        r(x)
        assert len(calls) == 1, calls
        fn, args = calls[0]
        rec["forward_calls"]["calls"][str(rows)] = {
            "fn": fn, "args": ["x" if a is x else names[id(a)] if isinstance(a, torch.Tensor) else a for a in args]}

    # tinychat's QuantLlamaMLP (the file alone: the tinychat.modules package __init__ pulls optional dependencies)
    spec = importlib.util.spec_from_file_location("_ref_fused_mlp", os.path.join(REF, "tinychat", "modules", "fused_mlp.py"))
    RF = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(RF)
    mk = lambda k, n: RQ.WQLinear(4, 128, k, n, False, "cpu", dtype=torch.float16)  # noqa: E731
    mlp = RF.QuantLlamaMLP(mk(256, 512), mk(512, 256), mk(256, 512))
    rec["quant_llama_mlp"] = {"shapes": [[256, 512], [512, 256], [256, 512]], "buffer_names": sorted(dict(mlp.named_buffers())),
                              "attributes": {a: getattr(mlp, a) for a in ("in_features", "intermediate_size", "out_features", "w_bit", "split_k_iters")}}

    # from_linear on a seeded input (fp16 and bf16)
    fl = {}
    rng = np.random.default_rng(20240611)
    K, N = 768, 96
    for name, dt in (("f16", torch.float16), ("bf16", torch.bfloat16)):
        w = (torch.from_numpy(rng.standard_normal((N, K), dtype=np.float32)) * 0.02).to(dt)
        fake, s, z = pseudo_quantize_tensor(w.clone(), n_bit=4, zero_point=True, q_group_size=128, get_scale_zp=True)
        lin = torch.nn.Linear(K, N, bias=True, dtype=dt)
        with torch.no_grad():
            lin.weight.data = fake.clone()
            lin.bias.data = (torch.from_numpy(rng.standard_normal(N, dtype=np.float32)) * 0.02).to(dt)
        q = RQ.WQLinear.from_linear(lin, 4, 128, False, s.clone(), z.clone())
        fl[name + "_weight"], fl[name + "_bias_in"], fl[name + "_s"], fl[name + "_z"] = bits(fake), bits(lin.bias.data), bits(s), bits(z)
        for k in ("qweight", "scales", "scaled_zeros", "bias"):
            fl[f"{name}_{k}"] = bits(getattr(q, k).detach())

    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "ref_qmodule.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    np.savez_compressed(os.path.join(OUT, "ref_from_linear.npz"), **fl)
    for fn in ("ref_qmodule.json", "ref_from_linear.npz"):
        print(fn, os.path.getsize(os.path.join(OUT, fn)))


if __name__ == "__main__":
    main()
