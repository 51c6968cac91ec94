"""K1 tile-resident kernel, tiles whose window holds the lattice's last row (EDGE form of the pair loop): the Philox row counter
comes from a per-wave distance to the wrap row, counted down, with per-lane compares only in the wave-iteration that straddles
it.  Where the wrap row falls in a tile's window depends on the halo depth (2k rows for k sweeps per generation) and on the tile
rows' heights, and how many tile rows a wave spans on the tile's width; each case below moves one of them.  Bit-exact against the
generic kernel (one thread per site, no tiles), one launch per call."""
import pytest

pytestmark = pytest.mark.gpu

T_C = 2.269185


@pytest.mark.parametrize("rows, cols, k, calls", [
    (4096, 4096, 0, (24, 21)),   # the bench lattice: 128 x 512 byte tiles; three generations, then a short last one
    (4096, 4096, 1, (5,)),       # halo of 2 rows: the wrap row is the window's second / last but one
    (4096, 4096, 2, (9,)),
    (4096, 4096, 5, (17,)),
    (2048, 2048, 0, (24, 21)),   # other tile shapes: narrower tiles, a wave spans more tile rows
    (1024, 1024, 0, (24, 21)),
    (4096, 8192, 0, (19,)),
    (4100, 4096, 0, (19,)),      # flexible cut: tile rows of unequal heights
    (6000, 6000, 0, (19,)),      # ... and a partial last tile column
    (8192, 8192, 0, (16,)),      # nibble planes, 512 x 512 tiles
])
def test_wrap_holding_tiles_equal_the_generic_kernel(rows, cols, k, calls):
    from tsu import _hip
    ctx = _hip.Context.default()
    table = _hip.ising2d_thresholds(1.0, 0.0, T_C)
    a = _hip.Lattice(rows, cols, True, ctx=ctx)
    b = _hip.Lattice(rows, cols, True, ctx=ctx)
    a.set_kernel(_hip.KERNEL_AUTO, k)
    b.set_kernel(_hip.KERNEL_GENERIC, 0)
    for lat in (a, b):
        lat.randomize(5)
        lat.set_thresholds(table)
    n0, s0 = a.launch_count(), 0
    for n in calls:
        a.sweep(n, 13, s0)
        b.sweep(n, 13, s0)
        s0 += n
    assert a.launch_count() - n0 == len(calls), "tile-resident: one launch per call"
    assert a.observables() == b.observables()
    assert (a.get_spins() == b.get_spins()).all()
    a.close()
    b.close()
