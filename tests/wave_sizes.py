"""The sizes with compile-time instances of the LDS-FFT tier, read from the table the kernels are instantiated from
(AC_WAVE_CT_SIZES in audiocodec_amd/csrc/ac_wave_v.h): a size added there is a test case without anybody copying a list."""

import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table(macro):
    lines = open(os.path.join(ROOT, "audiocodec_amd", "csrc", "ac_wave_v.h")).read().splitlines()
    at = next(i for i, ln in enumerate(lines) if re.match(r"#define %s\b" % macro, ln))
    body = []
    while lines[at].rstrip().endswith("\\"):     # the macro's continuation lines
        at += 1
        body.append(lines[at])
    return [(int(n), int(nt)) for n, nt in re.findall(r"AC_WAVE_CT\((\d+),\s*(\d+),", "\n".join(body))]


CT_TABLE = sorted(_table("AC_WAVE_CT_SIZES"))            # (filters_n, lanes per frame)
CT_SIZES = [n for n, _ in CT_TABLE]
CT_LANES = dict(CT_TABLE)
PCM_SIZES = sorted(n for n, _ in _table("AC_WAVE_PCM_SIZES"))

# the fused encode of the tier (k_enc_wave_v) has an instance where the masking model has a frame slot and the
# several-frames-per-wave kernels do not take every mono / stereo tensor: enc_instance() of ac_wave_enc.hip;
# test_kernel_coverage holds the list to the symbols the build emits
ENC_SIZES = [n for n in CT_SIZES if 108 <= n <= 4096 and n not in (128, 256, 512)]


def team_sizes(C):
    """Sizes whose team form (k_fwd_wave_c / k_inv_wave_c) takes C channels: a team is the ceil(C / 2) groups of lanes of one
    signal's channel pairs, and the kernels are bounded to 512 lanes where a frame takes more than a wave (team_geometry)."""
    CP = (C + 1) // 2
    return [n for n, nt in CT_TABLE if nt <= 64 or CP * nt <= 512]
