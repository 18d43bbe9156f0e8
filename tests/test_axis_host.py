"""The shift-axis layer without a GPU (sushi_amd/axis.py): an event's weight in the two scales its users take it in."""
from sushi_amd import axis


def test_event_weights_in_both_scales():
    """The joint search's weights sum to 1, the segmentation pass's to the number of events; each list bit for bit what its
    expression gives in float64, in that order of operations."""
    lens = [500, 900, 100]
    assert axis.event_weights("equal", lens, per_event=False) == [1.0 / 3, 1.0 / 3, 1.0 / 3]
    assert axis.event_weights("length", lens, per_event=False) == [500.0 / 1500.0, 900.0 / 1500.0, 100.0 / 1500.0]
    assert axis.event_weights("equal", lens, per_event=True) == [1.0, 1.0, 1.0]
    assert axis.event_weights("length", lens, per_event=True) == [1.0, 1.8, 0.2]
    assert axis.event_weights("length", lens, per_event=True) == [500.0 * 3 / 1500.0, 900.0 * 3 / 1500.0, 100.0 * 3 / 1500.0]
    for m in (3, 7, 33):
        got = axis.event_weights("equal", list(range(1, m + 1)), per_event=False)
        assert [w.hex() for w in got] == [(1.0 / m).hex()] * m
    for lens in ([500, 900, 100], [1, 2, 4, 7, 36000, 11, 3], list(range(5, 38))):
        total = float(sum(lens))
        got = axis.event_weights("length", lens, per_event=False)
        assert [w.hex() for w in got] == [(float(n) / total).hex() for n in lens]
    assert axis.event_weights([2, 0, 1], [5, 5, 5], per_event=False) == [2.0, 0.0, 1.0]
