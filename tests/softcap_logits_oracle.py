"""float64 statement of final-logit soft-capping (include/awq_cdna4.h: awq_logit_softcap, awq_lm_head_softcap, awq_lm_head_logprobs_softcap;
csrc/awq_softcap.hpp), on top of tests/lm_head_oracle.py:

    y = cap * tanh(z / cap),   z = the LM head's fp32 sum with the bias in it;   out T: y rounded once, nearest-even
    awq_lm_head_logprobs_softcap with round_logits: z is rounded to T, capped, and rounded to T once more

The bound.  The device evaluates fl(cap * device_tanh(fl(z / cap))).  tests/attn_softcap_oracle.py derives |device_tanh(y) - tanh(y)| <= 8.27 u
(u = 2^-24) for the function itself; the division in front is one relative rounding of the argument, at most 0.45 u behind the tanh
(max x sech^2 x = 0.4478), and the product behind is one relative rounding of a value no larger than cap: 8.27 + 0.45 + 1 = 9.72 <= C = 10.
|d tanh| <= 1, so an error b of z (lm_head_oracle.bound's (K + 1) u sum |xn w|, zero on the lattice) reaches y no larger than it was:

    |got - y| <= C * 2^-24 * cap + b      (+ ulp_T(|y| + that) / 2 where the result is rounded to T)

`mutant` switches one fault in:  nocap (y = z),  cap-before-bias (y = cap tanh((z - bias) / cap) + bias),  cap-after-round (out T only: the
rounding to T in front of the cap, y = T(cap tanh(T(z) / cap)))."""
import numpy as np

from tests import attn_softcap_oracle as A
from tests import lm_head_oracle as H

C = A.C
U = 2.0 ** -24
MUTANTS = ("nocap", "cap-before-bias", "cap-after-round")


def cap_f64(z, cap):
    with np.errstate(invalid="ignore"):
        return cap * np.tanh(np.asarray(z, dtype=np.float64) / cap)


def capped(z, cap, bias=None, out="f32", dtype_name="bf16", mutant=None):
    """float64 logits z [M, V] (bias included) -> the capped logits as the contract states them."""
    z = np.asarray(z, dtype=np.float64)
    if mutant == "nocap":
        y = z
    elif mutant == "cap-before-bias" and bias is not None:
        y = cap_f64(z - bias, cap) + bias
    elif mutant == "cap-after-round":
        y = cap_f64(H.round_T(z, dtype_name), cap)
    else:
        y = cap_f64(z, cap)
    return H.round_T(y, dtype_name) if out == "T" else y


def bound(y, cap, logit_bound=0.0, out="f32", dtype_name="bf16"):
    """per element, around the UNROUNDED float64 y"""
    b = np.zeros(np.shape(y)) + C * U * cap + np.asarray(logit_bound, dtype=np.float64)
    return b + (H.ulp_T(np.abs(y) + b, dtype_name) / 2 if out == "T" else 0.0)


def lm_head_case(case, cap, out="f32", mutant=None):
    """(value, unrounded y, bound) of awq_lm_head_softcap on an lm_head_oracle.build_lattice case (exact z: the logit bound is zero)."""
    bias = None if case["bias"] is None else H.f64(case["bias"])
    z = H.reference(case["x_store"], case["ldx"], case["M"], H.f64(case["w"]), bias, out="f32", dtype_name=case["dtype_name"])[0]
    y = cap_f64(z, cap)
    return capped(z, cap, bias, out, case["dtype_name"], mutant), y, bound(y, cap, 0.0, out, case["dtype_name"])
