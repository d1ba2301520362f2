"""The kernels of the wave-vector sums and of the time correlations keep their sums in registers: every template step of
kgrid_accumulate_kernel (csrc/structure_factor_kernels.hpp) with SkTerm (runs of 1 to 17 indices, 3-D float and 2-D double) and with
MdTerm (csrc/modes_kernels.hpp: runs of 1, 2, 3, 4 indices, 8 to 32 doubles of sums), of mode_corr_kernel (1, 2, 4 lags: 7 to 28
doubles) and of tc_accumulate_kernel (csrc/time_corr_kernels.hpp: 1, 2, 4, 8 lags) is in the built library and has no scratch
segment -- a private segment would mean that the sums are indexed at run time or spilled."""
import os
import re

import pytest

from test_source_rules import ROOT, _device_elfs, _kernel_descriptors

# (the mangled names: <length><name>I [NS_<length><term>E] Li<A>E [Lb<DIM3>E <T>] E ..)
_KGRID = r"\d+kgrid_accumulate_kernelINS_\d+%sELi(\d+)E%sE"
STEPS = {
    "kgrid_accumulate_kernel<SkTerm, A, true, float>": (_KGRID % ("SkTerm", "Lb1Ef"), {1, 2, 3, 5, 9, 13, 17}),
    "kgrid_accumulate_kernel<SkTerm, A, false, double>": (_KGRID % ("SkTerm", "Lb0Ed"), {1, 2, 3, 5, 9, 13, 17}),
    "kgrid_accumulate_kernel<MdTerm, A, true, float>": (_KGRID % ("MdTerm", "Lb1Ef"), {1, 2, 3, 4}),
    "mode_corr_kernel<A>": (r"\d+mode_corr_kernelILi(\d+)EE", {1, 2, 4}),
    "tc_accumulate_kernel<A>": (r"\d+tc_accumulate_kernelILi(\d+)EE", {1, 2, 4, 8}),
}


def test_modes_kernels_are_built_in_every_step_without_scratch():
    lib = os.path.join(ROOT, "coulomb_oscillators_amd", "libnbco_hip.so")
    if not os.path.exists(lib):
        pytest.skip("libnbco_hip.so is not built")
    blob = open(lib, "rb").read()
    found, bad = {k: set() for k in STEPS}, []
    for base in _device_elfs(blob):
        for name, props, scratch in _kernel_descriptors(blob, base):
            for k, (pattern, _) in STEPS.items():
                m = re.search(pattern, name)
                if m:
                    found[k].add(int(m.group(1)))
                    if scratch:
                        bad.append((name, scratch))
                    assert not props & 0x6, "%s reads the dispatch / queue packet" % name
    assert found == {k: steps for k, (_, steps) in STEPS.items()}, "template steps in the library: %s" % found
    assert not bad, "kernels with a scratch segment (bytes per lane): %s" % bad
