"""CapacityTracker (fresnel_amd/renderer.py): the host-only policy behind TileBasedRenderer(workspace="adaptive").  It turns the
duplicate demands that completed forwards reported (saved.counters[3]) into FgsDims.dup_capacity of the next forward.  No GPU:
the readback ring that feeds it on the device is exercised by tests/test_workspace_capacity.py."""
import math

import pytest

from fresnel_amd.renderer import CapacityTracker, quantise_capacity

WORST = 15_728_640  # config 3 (8 x 32 768 Gaussians at 512 x 512, 32 x 16 tiles)


def test_first_capacity_is_the_worst_case():
    t = CapacityTracker(WORST)
    assert t.capacity() == 0 and t.last_demand is None and t.overflows == 0
    assert (t.margin, t.window) == (1.25, 8) == (CapacityTracker.margin, CapacityTracker.window)


@pytest.mark.parametrize("demand", [1, 2, 7, 16, 17, 100, 3027, 4099, 65535, 65536, 65537, 1_234_017, 4_099_112, 10_309_213])
@pytest.mark.parametrize("margin", [1.0, 1.1, 1.25, 1.5])
def test_capacity_covers_margin_times_demand_in_steps_of_at_most_an_eighth(demand, margin):
    t = CapacityTracker(1 << 40, margin=margin)
    t.observe(demand)
    c = t.capacity()
    want = margin * demand
    assert c >= want, (c, want)
    # quantisation wastes at most one step of 12.5 % (plus the one unit of rounding margin x demand up to an integer)
    assert c <= math.ceil(want) * 1.125 + 1, (c, want)
    assert t.last_demand == demand


def test_quantisation_steps_are_at_most_an_eighth_and_few():
    prev = 0
    values = set()
    for x in list(range(1, 5000)) + [10 ** 6 + k * 997 for k in range(2000)]:  # ascending
        q = quantise_capacity(x)
        assert q >= x and q - x <= x / 8.0, (x, q)
        assert quantise_capacity(q) == q, "a quantised value is a fixed point"
        assert q >= prev, "monotonic"
        prev = q
        values.add(q)
    # a demand that wanders by a few percent settles on one size: 8 values per octave, not one per demand
    assert len([v for v in values if 1024 <= v < 2048]) == 8
    around = {quantise_capacity(int(1.25 * d)) for d in range(1_234_017 - 20_000, 1_234_017 + 20_000, 1000)}
    assert len(around) <= 2, around


def test_window_takes_the_maximum_and_drops_older_observations():
    t = CapacityTracker(WORST, window=3)
    t.observe(1000)
    assert t.capacity() == quantise_capacity(1250)
    t.observe(4000)
    t.observe(1000)
    assert t.capacity() == quantise_capacity(5000), "the maximum of the window, not the last demand"
    t.observe(1000)
    assert t.capacity() == quantise_capacity(5000), "4000 is the third-last observation: still inside a window of 3"
    t.observe(1000)
    assert t.capacity() == quantise_capacity(1250), "4000 is older than the window now"
    assert t.demands == [1000, 1000, 1000] and t.last_demand == 1000
    d = CapacityTracker(WORST)
    for k in range(20):
        d.observe(100 + k)
    assert len(d.demands) == 8 and d.demands[0] == 112


def test_a_capacity_that_reaches_the_worst_case_is_the_worst_case():
    t = CapacityTracker(18000)
    t.observe(3027)
    assert t.capacity() == 3840  # ceil(1.25 x 3027) = 3784 -> next multiple of 256
    t.observe(13000)             # 16 250 -> 16 384: still under the worst case
    assert t.capacity() == 16384
    t.observe(14400)             # 18 000 -> 18 432: reaches it
    assert t.capacity() == 0
    t2 = CapacityTracker(18000)
    t2.observe(18000)
    assert t2.capacity() == 0
    t3 = CapacityTracker(18000)
    t3.observe(0)                # an empty scene still gets a valid (non-zero = hinted) capacity
    assert t3.capacity() == 1


def test_an_overflow_observation_raises_the_next_capacity_above_its_demand():
    t = CapacityTracker(24000)
    t.observe(3027)
    c1 = t.capacity()
    assert c1 == 3840
    t.observe(4936, overflowed=True)  # the call ran with c1 and needed 4936
    assert t.overflows == 1 and t.last_demand == 4936
    c2 = t.capacity()
    assert c2 >= 1.25 * 4936 > 4936 > c1
    t.observe(4936)
    assert t.overflows == 1 and t.capacity() == c2, "steady state: one size"


def test_policy_attributes_are_validated_and_per_instance():
    t = CapacityTracker(1000, margin=2.0, window=1)
    assert (t.margin, t.window) == (2.0, 1) and CapacityTracker.margin == 1.25
    t.observe(100)
    t.observe(10)
    assert t.capacity() == quantise_capacity(20)
    t.margin = 1.0  # exposed as attributes
    assert t.capacity() == 10
    with pytest.raises(ValueError):
        CapacityTracker(1000, margin=0.9)
    with pytest.raises(ValueError):
        CapacityTracker(1000, window=0)
