"""Oracle-encoded containers and their damaged variants, shared by the host parser's tests and the device decoder's
(oracle only: nothing here needs a GPU)."""
import numpy as np

# (width, height, K, quality) of the oracle-encoded containers: mixed geometry, K and quality, more frames than slots
FRAMES = [(8, 8, 1, 2.0), (16, 8, 8, 3.5), (200, 120, 32, "max"), (1003, 517, 32, 3.5), (1920, 1080, 8, 6.0), (8, 8, 32, 6.0),
          (16, 8, 1, "max"), (200, 120, 8, 2.0), (1003, 517, 1, 6.0), (1920, 1080, 1, 2.0), (200, 120, 1, 3.5), (1003, 517, 8, "max")]


def corpus(oracle):
    """(index in FRAMES, container, [96 inputs]) of the eight containers below 100 000 bytes: 16 truncations, 64 single-bit flips
    anywhere, 16 in the header and the quantiser table"""
    for n in (0, 1, 2, 5, 6, 7, 8, 10):
        W, H, K, quality = FRAMES[n]
        octx = oracle.OracleContext(K, 8, 0.0 if quality == "max" else quality)
        blob = octx.encode_image(oracle.synth_frame(W, H, 100 + n), quant=np.ones((3, K)) if quality == "max" else None)
        assert len(blob) < 100000
        a = np.frombuffer(blob, np.uint8)
        rng = np.random.default_rng([20241102, n])
        xs = [bytes(a[:len(a) * k // 16]) for k in range(16)]
        for bits, count in ((8 * len(a), 64), (8 * (14 + 6 * K), 16)):
            for pos in rng.integers(0, bits, count):
                c = a.copy()
                c[pos // 8] ^= 1 << (pos % 8)
                xs.append(bytes(c))
        yield n, blob, xs
