"""CPU: every kernel the build emits is accounted for -- tests/kernel_coverage.txt lists, per gfx950 kernel symbol of the
library, the test files whose traced run launched it (tools/kernel_coverage.py; one rocprofv3 --kernel-trace run per test
file).  A kernel added, renamed or removed without a new trace fails here by name, as does a kernel no test file launches.

Needs the built library (as test_host.py does), no GPU."""

import ast
import importlib.util
import os
import re

from conftest import ROOT

from audiocodec_amd import _lib
from wave_sizes import CT_SIZES, ENC_SIZES, PCM_SIZES, team_sizes

MANIFEST = os.path.join(ROOT, "tests", "kernel_coverage.txt")

# Kernels a single-GPU test process cannot launch at all: mangled name -> one line of reason.  Nothing of the per-size
# families belongs here (a kernel a call or a documented switch reaches gets a test; one that nothing reaches is deleted).
EXEMPT = {
}
MAX_EXEMPT = 10


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_coverage", os.path.join(ROOT, "tools", "kernel_coverage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _manifest():
    return _tool().read_manifest(MANIFEST)


def _family(name):
    m = re.match(r"_ZN2ac(?:12_GLOBAL__N_1|L)?(\d+)", name)
    n = int(m.group(1))
    return name[m.end():m.end() + n]


def test_manifest_lists_exactly_the_kernels_of_the_library():
    syms = set(_tool().kernel_symbols(_lib.LIB_PATH))
    _, _, rows = _manifest()
    added, gone = sorted(syms - set(rows)), sorted(set(rows) - syms)
    assert not added and not gone, (
        "the library's kernels and tests/kernel_coverage.txt differ: trace the suite again (tools/README.md, kernel_coverage.py)\n"
        "  in the library, not in the manifest (%d): %s\n  in the manifest, not in the library (%d): %s"
        % (len(added), " ".join(added[:40]), len(gone), " ".join(gone[:40])))


def test_every_kernel_is_launched_by_a_test_file():
    _, codes, rows = _manifest()
    assert len(EXEMPT) <= MAX_EXEMPT, "EXEMPT holds %d kernels, at most %d may be exempt" % (len(EXEMPT), MAX_EXEMPT)
    for k, why in EXEMPT.items():
        assert isinstance(why, str) and why.strip() and "\n" not in why, "EXEMPT[%s] needs a one-line reason" % k
        assert k in rows, "EXEMPT names %s, which is no kernel of the manifest" % k
    for k, (_, head) in rows.items():
        assert head == "-" or set(head) <= set(codes), "row %s uses a code the header does not define: %s" % (k, head)
    never = sorted(k for k, (_, head) in rows.items() if head == "-" and k not in EXEMPT)
    assert not never, "%d kernels no test file launches (and not in EXEMPT):\n  %s" % (len(never), "\n  ".join(never))
    stale = sorted(k for k in EXEMPT if rows[k][1] != "-")
    assert not stale, "exempt, yet launched: %s" % stale


def test_sole_covers_named_by_the_manifest_exist():
    """A family whose instances only one test reaches: the header names that test (# sole-cover <kernel> <file>::<test>); a
    rename or removal of it fails here instead of silently uncovering the family.  Found by ast: importing the GPU modules
    is not needed to know a function is there."""
    header, _, rows = _manifest()
    families = {_family(k) for k in rows}
    named = [ln.split()[2:] for ln in header if ln.startswith("# sole-cover ")]
    assert named, "the manifest header names no sole cover"
    for fam, where in named:
        assert fam in families, "sole-cover names the kernel %s, which the library does not have" % fam
        mod, fn = where.split("::")
        tree = ast.parse(open(os.path.join(ROOT, "tests", mod + ".py")).read())
        defs = {n.name for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))}
        assert fn in defs, "%s (the only cover of %s) is gone from tests/%s.py" % (fn, fam, mod)


def test_size_lists_of_the_tests_equal_the_instances_of_the_build():
    """The parametrize lists come from the table in ac_wave_v.h (wave_sizes.py); the symbols say what the compiler made of it."""
    def smooth_half(N):
        h = N // 2
        for r in (2, 3, 5):
            while h % r == 0:
                h //= r
        return h == 1
    # test_gpu_parity.WAVE16_SIZES (by rule) plus the six powers of two of the wave-level kernels = the table
    rule = [N for N in range(16, 8193, 4) if smooth_half(N) and N not in (64, 128, 256, 512, 1024, 2048, 7500)]
    assert sorted(rule + [64, 128, 256, 512, 1024, 2048]) == CT_SIZES
    _, _, rows = _manifest()

    def sizes(family, rest=r""):
        return sorted(int(m.group(1)) for k in rows if _family(k) == family
                      for m in [re.search(r"k_\w+?ILi(\d+)E" + rest, k)] if m)
    enc = sizes("k_enc_wave_v")
    assert sorted(set(enc)) == ENC_SIZES and len(enc) == 2 * len(ENC_SIZES)          # stereo and mono rows
    for fam in ("k_fwd_wave_c", "k_inv_wave_c"):
        assert sizes(fam) == team_sizes(3), fam                                      # (no instance no channel count reaches)
    for fam in ("k_fwd_wave_v", "k_inv_wave_v"):
        got = sizes(fam)
        assert sorted(set(got) - {0}) == CT_SIZES, fam
        assert len(got) == 3 * (len(CT_SIZES) + 1) + 2 * len(PCM_SIZES), fam          # three layouts (+ run-time form), PCM rows
