"""Graph capture and the device entry points (run with -m gpu): refused, and harmless.

The pursuit launches of a process share the per-device queue words and scratch and are ordered by a chain of events recorded outside
any graph (mpcodec_context.cpp: run_persistent).  A captured launch would wait on an event recorded outside the capture, leave the
chain's event a captured one for the next plain launch, and a replay would take no part in the chain at all.  So a capturing stream is
refused: MPC_ERR_ARGUMENT with a message, before anything is enqueued (include/mpcodec.h, "Streams and graphs").  What is asserted:
the refusal of the encode and of the decode entry point inside torch.cuda.graph on a side stream (persistent path, quant == NULL, after
mpc_reserve), and in the same capture of every other entry point with a stream on a context that has made no call yet -- their first
call allocates and synchronises the device (the crop error word, the diff scratch, a job slot's buffers), which would end the capture
with an error, so the guard has to stand in front of that; that the capture ends cleanly and the graph replays what else was
captured; and that plain calls afterwards -- on the stream that was capturing and on another one, from this context, from a second
one and from the one that was only ever refused, i.e. along the shared event chain -- still give the oracle's records and the
oracle's pixels."""
import numpy as np
import pytest

import stream_order as so

pytestmark = pytest.mark.gpu

W, H, K = 197, 117, 8                      # 25 x 15 tiles, the right column and the bottom row partial
TX, TY = 25, 15
T = TX * TY


def test_a_capturing_stream_is_refused_and_nothing_is_broken(oracle):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests need a real MI355X (there is no CPU fallback)")
    import imageexperiments_amd as ia
    octx = oracle.OracleContext(K, 8, 3.5)
    QI = np.maximum(np.floor(octx.quant), 1.0)                      # integer tables: the header carries what the encoder used
    frames = {n: oracle.synth_frame(W, H, s) for n, s in (("A", 101), ("C", 303))}
    want = {n: so.device_records(octx.encode_tiles(px, quant=QI), K) for n, px in frames.items()}
    pixels = {n: oracle.decode_image(bytes(octx.encode_image(px, quant=QI))) for n, px in frames.items()}
    ctx, other, fresh = (ia.create_compression_context(K, 8, 3.5, device=0) for _ in range(3))
    try:
        for c in (ctx, other, fresh):
            c.set_quant(QI)
            c.reserve(T)
        S, S2 = torch.cuda.Stream(), torch.cuda.Stream()
        d_px = torch.from_numpy(frames["A"]).cuda()
        outs = [torch.full((n,), so.POISON, dtype=torch.uint8, device="cuda") for n in (T * 3 * 2, T * 3 * K * 4, T * 3 * 8, T * 3 * 4)]
        d_rgb = torch.full((H, W, 3), so.POISON, dtype=torch.uint8, device="cuda")
        marker = torch.zeros(16, dtype=torch.int32, device="cuda")
        d = torch.zeros(1 << 22, dtype=torch.uint8, device="cuda").data_ptr()      # room for any argument of the calls below
        weights = np.full((3, K), 1000, np.uint32)

        def first_calls(c, s):
            """every other entry point with a stream, with arguments that pass its checks"""
            return {
                "encode_batch_device": lambda: c.encode_batch_device(d, 2, 3 * W * H, W, H, 3 * W, 0, TY, d, d, stream=s),
                "histogram_device": lambda: c.histogram_device(d, d, T, d, stream=s),
                "interleave_stripe_device": lambda: c.interleave_stripe_device(d, d, W, H, 4, 11, d, d, stream=s),
                "container_job_begin": lambda: c.container_job_begin(2, d, d, W, H, stream=s),
                "records_to_container_device": lambda: c.records_to_container_device(d, d, W, H, stream=s),
                "crop_records_device": lambda: c.crop_records_device(d, d, W, H, None, 0, d, d, stream=s, check=False),
                "paste_records_device": lambda: c.paste_records_device(d, d, W, H, None, d, d, W, H, 0, 0, stream=s, check=False),
                "tile_diff_device": lambda: c.tile_diff_device(d, d, W, H, 0, d, d, stream=s),
                "pack_tiles_device": lambda: c.pack_tiles_device(d, W, H, 0, d, 70, 64, d, stream=s),
                "unpack_tiles_device": lambda: c.unpack_tiles_device(d, 0, d, 70, 64, d, W, H, stream=s, check=False),
                "scatter_records_device": lambda: c.scatter_records_device(d, d, d, 70, d, d, T, stream=s, check=False),
                "depth_profile_device": lambda: c.depth_profile_device(d, d, d, W, H, d, stream=s, check=False),
                "budget_allocate_device": lambda: c.budget_allocate_device(d, d, T, weights, 120, d, d, d, stream=s),
                "budget_allocate_floor_device": lambda: c.budget_allocate_floor_device(d, d, d, d, T, weights, 120, d, d, d, d, stream=s),
                "owed_tiles_device": lambda: c.owed_tiles_device(d, d, T, d, d, d, d, d, stream=s),
                "gather_records_device": lambda: c.gather_records_device(d, d, T, d, 100, d, d, 70, 64, d, d, stream=s, check=False),
                "distortion_device": lambda: c.distortion_device(d, d, d, W, H, d, d, stream=s),
                "debug_copy_gram_device": lambda: c.debug_copy_gram_device(0, 0, 1, 0, 1, d, stream=s),
                "debug_screen_probe_device": lambda: c.debug_screen_probe_device(0, 0, d, 1, d, d, stream=s),
                "debug_gram_device": lambda: ia.api.debug_gram_device(d, d, d, d, d, 1, 1, d, stream=s),
            }

        def encode(c, stream):
            c.encode_tiles_device(d_px.data_ptr(), W, H, 3 * W, 0, TY, *[t.data_ptr() for t in outs], stream=stream.cuda_stream)

        def decode(c, stream):
            c.decode_tiles_device(outs[0].data_ptr(), outs[1].data_ptr(), W, H, d_rgb.data_ptr(), stream=stream.cuda_stream)

        def check(name):
            for t, arr in zip(outs, want[name]):
                assert np.array_equal(t.cpu().numpy().view(arr.dtype).reshape(arr.shape), arr), name
            assert np.array_equal(d_rgb.cpu().numpy(), pixels[name]), name

        def plain(c, stream, name):
            d_px.copy_(torch.from_numpy(frames[name]).cuda())
            for t in outs:
                t.fill_(so.POISON)
            d_rgb.fill_(so.POISON)
            torch.cuda.synchronize()
            encode(c, stream)
            decode(c, stream)
            stream.synchronize()
            check(name)

        plain(ctx, S, "A")                                          # first calls made: nothing below allocates
        for t in outs:
            t.fill_(so.POISON)
        d_rgb.fill_(so.POISON)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=S):
            marker.add_(1)                                          # something of the caller's own in the graph
            for call in (encode, decode):
                with pytest.raises(ia.MpcError) as e:
                    call(ctx, torch.cuda.current_stream())
                assert e.value.status == ia.api.MPC_ERR_ARGUMENT and "captured" in str(e.value), str(e.value)
            for name, call in first_calls(fresh, torch.cuda.current_stream().cuda_stream).items():
                with pytest.raises(ia.MpcError) as e:
                    call()
                assert e.value.status == ia.api.MPC_ERR_ARGUMENT and "captured" in str(e.value), (name, str(e.value))
            marker.add_(1)
        # the capture ended cleanly: nothing ran yet, and a replay runs the caller's two kernels and nothing else
        torch.cuda.synchronize()
        assert int(marker[0]) == 0
        graph.replay()
        torch.cuda.synchronize()
        assert int(marker[0]) == 2
        assert all((t.cpu().numpy() == so.POISON).all() for t in outs) and (d_rgb.cpu().numpy() == so.POISON).all()
        # plain calls are as before: on the stream that was capturing, on another one, and from another context -- each launch waits
        # on the event the one before it recorded, whichever stream that was on
        plain(ctx, S, "C")
        plain(other, S2, "A")
        plain(ctx, S2, "C")
        plain(other, S, "A")
        # and the context that was only ever refused: its first real calls
        plain(fresh, S2, "C")
    finally:
        ctx.close()
        other.close()
        fresh.close()
