"""Shared parameter sets for the oracle and HIP parity tests."""
CUTOUT_CASES = {
    "config_test": (0.5, 450, dict(fixed=False, centered=True, window_width=1.0, window_depth=0.5,
                                   num_cutout_pts=56, padding_val=29.99, area_mode=True)),
    "dr_spaam": (0.5, 450, dict(fixed=True, centered=True, window_width=1.0, window_depth=0.5,
                                num_cutout_pts=56, padding_val=29.99, area_mode=True)),
    "defaults": (0.5, 450, dict(centered=False)),
    "stride2": (0.5, 450, dict(stride=2, fixed=True, window_width=1.3, window_depth=0.7,
                               num_cutout_pts=32, padding_val=29.99, area_mode=True)),
    "dense3600": (0.1, 3600, dict(fixed=True, centered=True, window_width=1.0, window_depth=0.5,
                                  num_cutout_pts=56, padding_val=29.99, area_mode=True)),
    "near": (0.5, 450, dict(fixed=True, centered=True, window_width=1.0, window_depth=0.5,
                            num_cutout_pts=56, padding_val=29.99, area_mode=True)),
}

# ---- kernel forms chosen by the size of the launch (tests/test_launch_size_gpu.py; tests/test_launch_plan.py checks
# on the host that these tables reach every form)
# conv families: (kernel_size, stride); "k3s1" runs through conv3_bn_lrelu, "k3s2" / "k1" through conv1d_bn_lrelu,
# "fused" through conv3_first_two (Ci = C1, the single-channel first unit computed in the kernel)
CONV_FAMILIES = {"k3s1": (3, 1), "k3s2": (3, 2), "k1": (1, 1), "fused": (3, 1)}

# (family, Ci, Co, L, pool, channels per workgroup, split K, quantised): the form each case must run.  quantised: the
# 64-channel form the launcher takes instead of 128 channels when a launch has fewer than two rounds of 128-channel
# workgroups.  Co = 130 / 70 leave a ragged last tile and take the element-wise weight path (Co % 4 != 0).
CONV_FORM_CASES = [
    ("k3s1", 64, 128, 56, False, 128, False, False),
    ("k3s1", 64, 130, 56, True, 128, False, False),
    ("k3s1", 64, 70, 28, False, 128, False, False),
    ("k3s1", 64, 70, 28, True, 64, False, False),
    ("k3s1", 128, 256, 14, False, 64, False, True),
    ("k3s1", 64, 130, 9, False, 32, False, False),
    ("k3s1", 128, 128, 28, True, 32, True, False),
    ("k3s1", 160, 130, 9, False, 32, True, False),
    ("k3s1", 160, 130, 9, False, 64, True, False),
    ("k3s1", 512, 256, 7, False, 64, True, False),
    ("k3s2", 64, 128, 225, False, 128, False, False),
    ("k3s2", 33, 130, 57, False, 128, False, False),
    ("k3s2", 64, 70, 57, False, 64, False, False),
    ("k3s2", 64, 130, 113, False, 64, False, True),
    ("k3s2", 1, 64, 451, False, 32, False, False),
    ("k1", 128, 256, 64, True, 128, False, False),
    ("k1", 129, 70, 50, False, 64, False, False),
    ("k1", 64, 130, 7, False, 32, False, False),
    ("fused", 64, 128, 56, True, 128, False, False),
    ("fused", 64, 64, 56, False, 64, False, False),
    ("fused", 64, 130, 28, False, 64, False, True),
    ("fused", 20, 130, 48, False, 32, False, False),
]

# one launch that writes more than 2^30 output elements (64-bit output offsets): (family, Ci, Co, L, pool, S)
CONV_WIDE_CASE = ("k3s1", 64, 128, 56, False, 160000)

# spatial attention at E = 128, F = 3584 (256 channels x 14 points), window 11: (B, N, forward segment, fused backward
# segment); every case is also compared with B = 1 launches of some of its rows (the shortest segments)
ATTENTION_E, ATTENTION_F, ATTENTION_W = 128, 3584, 11
ATTENTION_CASES = [(32, 450, 29, 29), (64, 450, 57, 57), (256, 450, 225, 225), (439, 450, 450, 450),
                   (256, 451, 226, 226)]

# training tail at the reference's batch: (S, groups, C, L, pool) for bn_lrelu_pool_*, (S, Ci, Co, L) for conv3_wgrad
BN_TAIL_CASES = [(18000, 5, 64, 56, False), (72000, 1, 64, 56, True)]
WGRAD_CASES = [(18000, 64, 128, 56), (3600, 256, 256, 14)]


def conv_quantised(S, Co, L, stride, plan):
    """True when `plan` (ops.conv1d_plan of S sequences) is the 64-channel form that a 128-channel launch was
    narrowed to: enough workgroups to fill the chip at 128 channels, fewer than two rounds of them."""
    Lc = L if stride == 1 else (L + 1) // 2
    gx = ((S * Lc + 31) // 32 + 3) // 4                 # workgroups along the columns (32 columns x 4 waves)
    return (not plan["split_k"] and plan["channels_per_workgroup"] == 64 and Co > 64
            and gx * ((Co + 127) // 128) >= 256)


def conv_case_batch(conv1d_plan, case, s_min=24, s_max=1 << 15):
    """The smallest sequence count S >= s_min at which `case` (a CONV_FORM_CASES row) runs its form, found with the
    host-only plan query ops.conv1d_plan."""
    family, Ci, Co, L, pool, cpw, split, quantised = case
    kernel, stride = CONV_FAMILIES[family]
    for S in range(s_min, s_max):
        p = conv1d_plan(S, Ci, Co, L, kernel, stride, pool, family == "fused")
        if (p["split_k"], p["channels_per_workgroup"]) == (split, cpw) and \
                conv_quantised(S, Co, L, stride, p) == quantised:
            return S
    raise ValueError("no S in [%d, %d) runs the form of %s" % (s_min, s_max, case))
