"""streams.hop / streams.adopt: the one stream hop of the training steps (DetectorTrainer's weight gradients, RPN-stream work and filter
preparation, AxisTrainer's T tower), on the trainer that owns the stream cursor."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 1 << 20
SLEEP = 5_000_000  # device clock ticks: milliseconds at least, far longer than the host needs to enqueue what follows


def test_hop_orders_reads_keeps_allocations_and_restores_the_stream(hip_model):
    from articulation3d_amd import streams
    from articulation3d_amd.training import DetectorTrainer

    tr = DetectorTrainer(hip_model, seed=3)
    tr._begin_step(False)
    main, side = torch.cuda.current_stream(), streams.side(1)
    assert tr._cur_stream == main and side != main
    x = torch.zeros(N, device="cuda")
    _ = (x * 2 + 1) + 1  # (the kernels used below are loaded before anything is timed against a sleep)
    torch.cuda.synchronize()
    seen = []

    def reader():
        seen.append((torch.cuda.current_stream(), tr._cur_stream))
        return x * 2 + 1

    # 1. the side stream reads what the main stream writes behind a sleep: it must see the written values
    torch.cuda._sleep(SLEEP)
    x.fill_(3.0)
    y, done = streams.hop(tr, side, (x,), tr._next_event, reader, done=True)
    assert seen == [(side, side)] and torch.cuda.current_stream() == main and tr._cur_stream == main
    # 2. what the hop allocated is consumed on the main stream behind the join (and behind another sleep), then freed while that read is
    # pending: neither a new tensor of the main stream nor one of the side stream -- whose allocator owns the block -- may land on it
    main.wait_event(done)
    streams.adopt([y], main)
    torch.cuda._sleep(SLEEP)
    z = y + 1
    del y
    w = torch.full((N,), 5.0, device="cuda")
    with torch.cuda.stream(side):
        y2 = torch.full((N,), 9.0, device="cuda")
    torch.cuda.synchronize()
    assert bool((z == 8.0).all()) and bool((w == 5.0).all()) and bool((y2 == 9.0).all())
    # ... and once more through the hop, on the blocks the first round has released
    del z, w, y2
    torch.cuda._sleep(SLEEP)
    x.fill_(4.0)
    y, done = streams.hop(tr, side, (x,), tr._next_event, reader, done=True)
    main.wait_event(done)
    streams.adopt([y], main)
    z = y + 1
    del y
    w = torch.full((N,), 6.0, device="cuda")
    torch.cuda.synchronize()
    assert bool((z == 10.0).all()) and bool((w == 6.0).all())

    # 3. an exception inside the callable leaves both the process's current stream and the trainer's cursor restored
    def broken():
        assert torch.cuda.current_stream() == side and tr._cur_stream == side
        raise RuntimeError("inside the hop")

    with pytest.raises(RuntimeError, match="inside the hop"):
        streams.hop(tr, side, (x,), tr._next_event, broken, done=True)
    assert torch.cuda.current_stream() == main and tr._cur_stream == main
    # (no side stream: the callable runs inline and there is no event to wait for)
    assert streams.hop(tr, None, (x,), tr._next_event, lambda: tr._cur_stream, done=True) == (main, None)
    torch.cuda.synchronize()
