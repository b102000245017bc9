"""The inputs of tests/test_ctc_range_gpu.py, judged by the log-domain oracle alone (no GPU): every `hazard` utterance is feasible, has
a finite loss, and needs a lattice that reaches further below its column maxima than fp64 can (exp(-745) is below the smallest
denormal) - for the final states and, on at least one frame, for every alpha * beta product (batch F: for the products only, its final
states are in range); every control utterance stays above exp(-600) on both counts.  Without this the GPU tests would not leave the regime the linear-domain lattice was built for."""
import numpy as np
import pytest
import torch

from tests import ctc_range_cases as C

PAST, INSIDE = -745.0, -600.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", C.RANGE_NAMES)
def test_hazard_cases_leave_the_fp64_range_and_controls_do_not(name, dtype):
    c =C.range_case(name, dtype)
    for b, hz in enumerate(c.hazard):
        Tb, L = int(c.in_len[b]), int(c.lab_len[b])
        lab = c.labels[b, :L]
        feasible = Tb >= L + C.repeats(lab)
        nll, tail, frame = C.margins(c.logits[b, :Tb], lab)
        print(f"{name}[{b}] T={Tb} L={L}: nll {nll:.4f}, final states / column max = exp({tail:.1f}), worst frame = exp({frame:.1f})")
        if hz is None:
            assert not feasible and nll == np.inf
            continue
        assert feasible and np.isfinite(nll)
        if hz == "frames":
            assert tail > INSIDE and frame < PAST, (name, b, tail, frame)
        elif hz:
            assert tail < PAST and frame < PAST, (name, b, tail, frame)
        else:
            assert tail > INSIDE and frame > INSIDE, (name, b, tail, frame)


def test_exactly_feasible_batch_has_one_frame_per_state():
    c = C.range_case("B")
    assert c.in_len[0] == c.lab_len[0] + C.repeats(c.labels[0, : c.lab_len[0]]) == c.logits.shape[1] == 96
