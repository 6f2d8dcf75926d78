"""Kernel name -> kind of the greedy decode's step kernels, shared by the trace tools
(dec_gaps, dec_steps_csv, dec_overlap, trace_decode, trace_steps).

Both families of decoder.hip are listed: the big-tile step kernels and the co-resident
(`_slim_kernel`) ones the shipped library launches.  Keys are substrings of the demangled kernel
name in a rocprofv3 kernel trace.
"""

STEP_KINDS = (
    ("dec_pred_kernel<0", "pred0"), ("dec_pred_slim_kernel<0", "pred0"), ("dec_pred0h_slim", "pred0"),
    ("dec_pred_kernel<1", "pred1"), ("dec_pred1x_slim", "pred1"),
    ("dec_g_kernel", "g"), ("dec_g_slim", "g"),
    ("dec_joint_kernel", "joint"), ("dec_joint_slim", "joint"),
)


def step_kind(name):
    """pred0 / pred1 / g / joint for a step kernel's name, None for any other kernel."""
    for key, kind in STEP_KINDS:
        if key in name:
            return kind
    return None
