"""CPU checks of the polyploid entry points of the C ABI (no GPU needed): the set count of the full enumeration."""
import math

from rpvg_amd import hip


def test_full_set_count_is_the_multiset_count():
    L = hip.lib()
    for g in range(1, 9):
        assert L.rpvg_hip_full_set_count(0, g) == 0
        for G in range(1, 50):
            assert L.rpvg_hip_full_set_count(G, g) == math.comb(G + g - 1, g), (G, g)
    assert L.rpvg_hip_full_set_count(200, 8) == math.comb(207, 8)  # over the bound of one problem, still exact
    assert L.rpvg_hip_full_set_count(4_000_000_000, 8) == 2 ** 64 - 1  # saturates


def test_full_posteriors_is_bound():
    assert "rpvg_hip_group_full_posteriors" in hip.EXPORTS and "rpvg_hip_full_set_count" in hip.EXPORTS
    assert hasattr(hip.DeviceGroups, "full_posteriors")
