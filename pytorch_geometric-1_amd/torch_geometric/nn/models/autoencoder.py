"""GAE / VGAE (PyG 1.4.x nn.models.autoencoder [U]) on the native link kernels.

Upstream's InnerProductDecoder gathers z[row] and z[col] into two [E, C] arrays,
and recon_loss draws its negatives on the host.  Here the decoder is
mi355_mp.ops.edge_score (a lane group per edge, no per-edge rows), the stock
recon_loss is the fused mi355_mp.ops.link_loss over negatives from the native
sampler, and test() computes ROC-AUC and average precision itself (float64, on
the host), so nothing on this path needs scikit-learn.
"""
import numpy as np
import torch

from mi355_mp import ops as _ops

from ..inits import reset
from ...utils.train_test_split_edges import train_test_split_edges

EPS = 1e-15
MAX_LOGVAR = 10


def roc_auc_score(y_true, y_score):
    """Area under the ROC curve from ranks (Mann-Whitney), tied scores sharing
    their average rank; float64."""
    y = np.asarray(y_true).astype(bool).ravel()
    s = np.asarray(y_score, dtype=np.float64).ravel()
    n_pos, n_neg = int(y.sum()), int((~y).sum())
    if n_pos == 0 or n_neg == 0:
        raise ValueError("roc_auc_score needs both classes")
    vals, inv, cnt = np.unique(s, return_inverse=True, return_counts=True)
    end = np.cumsum(cnt).astype(np.float64)          # last 1-based rank of each distinct score
    rank = (end - (cnt - 1) / 2.0)[inv]
    return float((rank[y].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * float(n_neg)))


def average_precision_score(y_true, y_score):
    """sum_n (R_n - R_{n-1}) P_n over the distinct thresholds, from the highest
    score down; float64."""
    y = np.asarray(y_true).astype(bool).ravel()
    s = np.asarray(y_score, dtype=np.float64).ravel()
    n_pos = int(y.sum())
    if n_pos == 0:
        raise ValueError("average_precision_score needs a positive")
    order = np.argsort(-s, kind="stable")
    s, y = s[order], y[order]
    last = np.r_[np.nonzero(s[1:] != s[:-1])[0], s.size - 1]   # last position of each distinct score
    tp = np.cumsum(y)[last].astype(np.float64)
    precision = tp / (last + 1.0)
    recall = tp / n_pos
    return float(np.sum(np.diff(np.r_[0.0, recall]) * precision))


class InnerProductDecoder(torch.nn.Module):
    r"""sigma(z_i . z_j) for the node pairs of edge_index (forward) or for all
    pairs (forward_all)."""

    def forward(self, z, edge_index, sigmoid=True):
        return _ops.edge_score(z, edge_index, sigmoid)

    def forward_all(self, z, sigmoid=True):
        adj = torch.matmul(z, z.t())
        return torch.sigmoid(adj) if sigmoid else adj


class GAE(torch.nn.Module):
    def __init__(self, encoder, decoder=None):
        super(GAE, self).__init__()
        self.encoder = encoder
        self.decoder = InnerProductDecoder() if decoder is None else decoder
        GAE.reset_parameters(self)

    def reset_parameters(self):
        reset(self.encoder)
        reset(self.decoder)

    def encode(self, *args, **kwargs):
        return self.encoder(*args, **kwargs)

    def decode(self, *args, **kwargs):
        return self.decoder(*args, **kwargs)

    def split_edges(self, data, val_ratio=0.05, test_ratio=0.1):
        return train_test_split_edges(data, val_ratio, test_ratio)

    def recon_loss(self, z, pos_edge_index):
        r"""-log(decoder(pos) + EPS).mean() - log(1 - decoder(neg) + EPS).mean(), the
        negatives drawn against pos_edge_index with its self loops removed and one
        loop per node added, as upstream (the sampler's key table is built that way
        once per pos_edge_index tensor).  With the stock decoder both terms and
        their gradient are the fused mi355_mp.ops.link_loss; a custom decoder is
        called as upstream composes it."""
        neg_edge_index = _ops.negative_sample(pos_edge_index, z.size(0), loops=True)
        if type(self.decoder) is InnerProductDecoder:
            return _ops.link_loss(z, pos_edge_index, neg_edge_index, neg_trusted=True)
        pos_loss = -torch.log(self.decoder(z, pos_edge_index, sigmoid=True) + EPS).mean()
        neg_loss = -torch.log(1 - self.decoder(z, neg_edge_index, sigmoid=True) + EPS).mean()
        return pos_loss + neg_loss

    def test(self, z, pos_edge_index, neg_edge_index):
        """(ROC-AUC, average precision) of the decoder's scores for the positive
        against the negative pairs."""
        pos_y = z.new_ones(pos_edge_index.size(1))
        neg_y = z.new_zeros(neg_edge_index.size(1))
        y = torch.cat([pos_y, neg_y], dim=0)
        pos_pred = self.decoder(z, pos_edge_index, sigmoid=True)
        neg_pred = self.decoder(z, neg_edge_index, sigmoid=True)
        pred = torch.cat([pos_pred, neg_pred], dim=0)
        y, pred = y.detach().cpu().numpy(), pred.detach().cpu().numpy()
        return roc_auc_score(y, pred), average_precision_score(y, pred)


class VGAE(GAE):
    def __init__(self, encoder, decoder=None):
        super(VGAE, self).__init__(encoder, decoder)

    def reparametrize(self, mu, logvar):
        if self.training:
            return mu + torch.randn_like(logvar) * torch.exp(logvar)
        return mu

    def encode(self, *args, **kwargs):
        self.__mu__, self.__logvar__ = self.encoder(*args, **kwargs)
        self.__logvar__ = self.__logvar__.clamp(max=MAX_LOGVAR)
        return self.reparametrize(self.__mu__, self.__logvar__)

    def kl_loss(self, mu=None, logvar=None):
        mu = self.__mu__ if mu is None else mu
        logvar = self.__logvar__ if logvar is None else logvar.clamp(max=MAX_LOGVAR)
        return -0.5 * torch.mean(torch.sum(1 + logvar - mu ** 2 - logvar.exp(), dim=1))
