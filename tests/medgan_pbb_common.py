"""Host side of the tests of the partial-black-box attack on medGAN tables: generator + decoder restated in torch from the state dicts
(BatchNorm1d in eval mode, eps 1e-3; gan_models/medgan/model.py:13-73 of the reference), and the inputs the GPU tests share."""
import numpy as np
import torch

# (n, F) of the codes tests: F = 1, 65, 129 sit at the edges of the decoder's column padding, (257, 128) has none and more than one row
# tile, 1071 is BASELINE configs[4]
SHAPES = [(1, 1), (5, 65), (3, 129), (257, 128), (33, 1071)]
WEIGHT_SEEDS = {1071: 555, 1: 601, 65: 665, 128: 730, 129: 730}


def weights_seed(F):
    """the seed of synth.medgan_state_dicts for a table of F columns"""
    return WEIGHT_SEEDS[F]


def latents(n, F):
    return np.random.default_rng(7000 + 10 * F + n).standard_normal((n, 128)).astype(np.float32)


class Net:
    """the generator and the decoder before the threshold, in `dtype`"""

    def __init__(self, gsd, asd, binary, dtype=torch.float64):
        t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)                       # noqa: E731
        self.dtype, self.binary = dtype, bool(binary)
        self.blocks = [[t(gsd["%s.%s" % (name, k)]) for k in ("0.weight", "0.bias", "1.weight", "1.bias", "1.running_mean", "1.running_var")]
                       for name in ("gen_block1", "gen_block2")]
        self.w3, self.b3 = t(asd["decoder.0.weight"]), t(asd["decoder.0.bias"])

    def _block(self, x, block, act):
        w, b, gamma, beta, mean, var = self.blocks[block]
        h = torch.nn.functional.linear(x, w, b)
        return x + act((h - mean) / torch.sqrt(var + 1e-3) * gamma + beta)

    def hidden(self, z):
        """Generator.forward -> numpy [n, 128]"""
        with torch.no_grad():
            x = torch.from_numpy(np.asarray(z)).to(self.dtype)
            return self._block(self._block(x, 0, torch.relu), 1, torch.tanh).numpy()

    def decode(self, hidden):
        """Autoencoder.decode of hidden rows -> numpy [n, F]"""
        with torch.no_grad():
            lin = torch.nn.functional.linear(torch.from_numpy(np.asarray(hidden)).to(self.dtype), self.w3, self.b3)
            return (torch.sigmoid(lin) if self.binary else torch.relu(lin)).numpy()

    def dot_magnitude(self, hidden):
        """sum_k |hidden_k| |W_fk| + |b_f|: what the rounding of the decoder's dot product scales with -> numpy [n, F]"""
        with torch.no_grad():
            return (torch.from_numpy(np.asarray(hidden)).to(self.dtype).abs() @ self.w3.abs().T + self.b3.abs()).numpy()


def hamming(rows_a, rows_b):
    """S of the exact search on 0/1 tables: sum (a - b)^2 in integers, per row"""
    a, b = np.asarray(rows_a).astype(np.int64), np.asarray(rows_b).astype(np.int64)
    return ((a - b) ** 2).sum(axis=1)
