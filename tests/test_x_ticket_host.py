"""Host arithmetic of the ticketed forward X pass (csrc/dfft_kernels.h, x_ticket_count; csrc/dfft_fft_impl.h, fft_tiles_kernel with
Tune::TICKET), no GPU: a plan never resets its counter, so the host's running base must move on by exactly what a launch draws."""
import ctypes as C
import random

import pytest

M32 = 1 << 32


@pytest.fixture(scope="module")
def base_after(native_lib):
    """dfft_x_ticket_base_after(base, ntiles, grid, launches): the library's stepping of the ticket base.  A test hook, not part of the
    C-ABI of include/dfft.h, so it is bound here."""
    f = native_lib.dfft_x_ticket_base_after
    f.restype, f.argtypes = C.c_uint, [C.c_uint, C.c_longlong, C.c_longlong, C.c_longlong]
    return f


def _model_launch(counter, base, ntiles, grid, rng):
    """The kernel's loop, one generator per workgroup, interleaved at random: draws two tickets, then one more per tile it processes,
    and stops when its current ticket lies past the end.  Tickets are decoded as (counter value - base) mod 2^32, as the kernel does.
    Returns (counter after the launch, tiles in the order they were processed, end tickets per workgroup)."""
    state = {"ctr": counter}
    tiles, ends = [], [0] * grid

    def take(w):
        t = (state["ctr"] - base) % M32
        state["ctr"] = (state["ctr"] + 1) % M32
        if t >= ntiles:
            ends[w] += 1
        return t

    def workgroup(w):
        first = take(w)
        yield
        second = take(w)
        yield
        while first < ntiles:
            third = take(w)
            yield
            tiles.append(first)
            first, second = second, third

    live = [workgroup(w) for w in range(grid)]
    while live:
        g = rng.choice(live)
        try:
            next(g)
        except StopIteration:
            live.remove(g)
    return state["ctr"], tiles, ends


@pytest.mark.parametrize("ntiles,grid", [(64, 256), (320, 256), (1024, 256), (1, 1), (5, 2), (256, 256), (32768, 256)])
def test_a_launch_draws_one_ticket_per_tile_and_two_end_tickets_per_workgroup(base_after, ntiles, grid):
    rng = random.Random(ntiles * 1000 + grid)
    base = M32 - ntiles // 2 - 3  # the counter wraps in the middle of the launch
    ctr, tiles, ends = _model_launch(base, base, ntiles, grid, rng)
    assert sorted(tiles) == list(range(ntiles))
    assert ends == [2] * grid
    assert ctr == (base + ntiles + 2 * grid) % M32
    assert base_after(base, ntiles, grid, 1) == ctr


def test_ticket_base_steps_per_launch_and_wraps(base_after):
    f = base_after
    assert f(0, 32768, 256, 0) == 0
    assert f(0, 32768, 256, 1) == 32768 + 512
    assert f(7, 320, 256, 3) == 7 + 3 * (320 + 512)
    step = 32768 + 512
    for g in (1, 129055, 129056, 129057, 1000003):  # 2^32 / 33280 = 129055.5...: around the first wrap and far beyond it
        assert f(0, 32768, 256, g) == (g * step) % M32, g
    assert f(M32 - 1, 64, 64, 1) == (M32 - 1 + 64 + 128) % M32
    # launches of different shapes from one plan's point of view never happen, but two launches in a row must chain: the model started
    # at the stepped base processes every tile again
    rng = random.Random(5)
    base = M32 - 700
    for _ in range(3):
        ctr, tiles, ends = _model_launch(base, base, 320, 256, rng)
        assert sorted(tiles) == list(range(320)) and ends == [2] * 256
        assert ctr == f(base, 320, 256, 1)
        base = ctr
