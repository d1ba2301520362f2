"""The kernels of the collective modes keep their sums in registers (csrc/modes_kernels.hpp): every template step of
modes_accumulate_kernel (runs of 1, 2, 3, 4 indices: 8 to 32 doubles of sums) and of mode_corr_kernel (1, 2, 4 lags: 7 to 28 doubles)
is in the built library and has no scratch segment -- a private segment would mean that the sums are indexed at run time or spilled."""
import os
import re

import pytest

from test_source_rules import ROOT, _device_elfs, _kernel_descriptors

STEPS = {"modes_accumulate_kernel": {1, 2, 3, 4}, "mode_corr_kernel": {1, 2, 4}}


def test_modes_kernels_are_built_in_every_step_without_scratch():
    lib = os.path.join(ROOT, "coulomb_oscillators_amd", "libnbco_hip.so")
    if not os.path.exists(lib):
        pytest.skip("libnbco_hip.so is not built")
    blob = open(lib, "rb").read()
    found, bad = {k: set() for k in STEPS}, []
    for base in _device_elfs(blob):
        for name, props, scratch in _kernel_descriptors(blob, base):
            for k in STEPS:
                m = re.search(r"\d+%sILi(\d+)E" % k, name)   # (the mangled name: <length><name>I Li<A>E ..)
                if m:
                    found[k].add(int(m.group(1)))
                    if scratch:
                        bad.append((name, scratch))
                    assert not props & 0x6, "%s reads the dispatch / queue packet" % name
    assert found == STEPS, "template steps in the library: %s" % found
    assert not bad, "modes kernels with a scratch segment (bytes per lane): %s" % bad
