"""CPU: the case table of test_chip_scale.py covers every (entry point, path) pair it is meant to, at a chip-filling launch.
Removing a case then fails here instead of quietly shrinking what the GPU suite checks."""

import math

from chip_scale_inputs import CLIP_SAMPLES, MIN_CLIPS, MIN_WORKGROUPS
from test_chip_scale import CASES

FWD, INV = "mdct.transform", "mdct.inverse_transform"
TON, THR = "psy.tonality", "psy.global_masking_threshold"

REQUIRED = {
    # filter bank, float32: every tier, the per-frame-offset sizes, the team form and the strided pairs
    (FWD, "tier3"), (INV, "tier3"), (FWD, "tier2"), (INV, "tier2"), (FWD, "tier2_frame_offsets"),
    (INV, "tier2_frame_offsets"), (INV, "tier2_vs_oracle"), (INV, "tier2_frame_offsets_vs_oracle"),
    (FWD, "tier1"), (INV, "tier1"), (FWD, "tier0"), (INV, "tier0"),
    (FWD, "team"), (INV, "team"), (FWD, "strided_pairs"), (INV, "strided_pairs"),
    # masking model: each spreading form of tier 2, the run kernels at every granule-register count, their team form (and
    # at R = 4 forced), the strided pairs, the band walk, tier 0
    *[(e, p) for e in (TON, THR) for p in ("tier2_f32", "tier2_bf16_mfma", "tier2_bf16x2_mfma", "runs_R1", "runs_R2",
                                             "runs_R4", "runs_R8", "runs_R16", "runs_R32", "runs_team", "runs_team_R4",
                                             "runs_strided_pairs", "band_walk", "tier0")],
    # fused encode
    ("codec.encode", "fused_wave"), ("codec.encode", "fused_lds"), ("codec.encode", "fused_lds_frame_offsets"),
    ("codec.encode", "fused_forced"), ("codec.encode", "two_launch"), ("codec.encode", "multichannel"),
    ("codec.encode", "wave_two_launch"), ("codec.decode", "after_fused"), ("codec.decode", "after_wave"),
    ("codec.decode", "multichannel"),
    # 2-byte dtypes
    ("bf16.encode", "wave"), ("bf16.decode", "wave"), ("bf16.encode", "lds"), ("bf16.decode", "lds"),
    ("f16.filter_bank", "lds"), ("f16.filter_bank", "wave"),
    # streaming
    ("stream.run", "duplex"), ("stream.run", "lds_chain"),
    # quantiser family
    ("psy.quantize", "rows"), ("psy.dequantize", "rows"), ("psy.pack", "multi_tile_scan"), ("psy.unpack", "multi_tile_scan"),
    ("psy.quantize_to_budget", "register_scalar"), ("psy.quantize_to_budget", "register_per_row"),
    ("psy.quantize_to_budget", "reread_scalar"), ("psy.quantize_to_budget", "reread_per_row"),
    ("codec.decode_quantized", "one_launch"), ("codec.decode_quantized", "two_launches"),
    ("codec.decode_packed", "one_launch"), ("codec.decode_packed", "two_launches"),
}

# sizes the issue of this module names per path (a size may move between cases, not out of the table)
REQUIRED_SIZES = {
    (FWD, "tier3"): {(1024, 1), (1024, 2), (2048, 1), (2048, 2)},
    (FWD, "tier2"): {480, 960, 1920, 4096, 8192},
    (FWD, "tier2_frame_offsets"): {1152, 2304},
    (FWD, "tier1"): {250, 810},
    (FWD, "team"): {(960, 6), (1024, 3)},
    (FWD, "strided_pairs"): {(512, 5)},
    (TON, "tier2_bf16x2_mfma"): {1024, 2048},
    ("codec.encode", "fused_wave"): {(n, c) for n in (64, 128, 256, 512, 1024, 2048) for c in (1, 2)
                                     if (n, c) not in ((64, 1), (128, 2), (256, 1), (2048, 1))},
    ("codec.encode", "wave_two_launch"): {(2048, 1)},
    ("f16.filter_bank", "lds"): {960, 4096},
}


def test_every_path_has_a_chip_filling_case():
    covered = {pair for c in CASES for pair in c["covers"]}
    missing = REQUIRED - covered
    assert not missing, "paths without a chip-scale case: %s" % sorted(missing)
    for pair, sizes in REQUIRED_SIZES.items():
        have = {(c["N"], c["C"]) for c in CASES if pair in c["covers"]}
        for s in sizes:
            ok = s in have if isinstance(s, tuple) else any(n == s for n, _ in have)
            assert ok, "%s lost its case at %s" % (pair, s)


def test_every_case_fills_the_chip():
    ids = [c["id"] for c in CASES]
    assert len(ids) == len(set(ids))
    for c in CASES:
        B, K, N, C = c["B"], c["K"], c["N"], c["C"]
        K = c.get("K_stream", K)
        assert B >= MIN_CLIPS and B * K * N >= MIN_CLIPS * CLIP_SAMPLES - MIN_CLIPS * N, c["id"]
        pairs = (C + 1) // 2 if C > 1 else 0.5
        assert math.ceil(B * (K + 1) * pairs) >= MIN_WORKGROUPS, c["id"]
