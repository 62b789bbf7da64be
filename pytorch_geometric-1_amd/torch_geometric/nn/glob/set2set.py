import torch
from mi355_mp import ops as _ops

from ._readout import fused_layout, recipe


class Set2Set(torch.nn.Module):
    r"""The global pooling operator of `"Order Matters: Sequence to sequence for
    Sets" <https://arxiv.org/abs/1511.06391>`_ (PyG 1.4.3 nn.glob.Set2Set):

        q_t = LSTM(q*_{t-1}),  a_{i,t} = softmax_graph(x_i . q_t),
        r_t = sum_i a_{i,t} x_i,  q*_t = q_t || r_t

    The LSTM is torch's; everything from the scores to q*_t is one fused native
    call per step for a sorted float32 batch on the GPU, and upstream's recipe on
    the native softmax and scatter ops otherwise.

    Args:
        in_channels (int): size of each input sample.
        processing_steps (int): number of iterations T.
        num_layers (int): number of recurrent layers. (default: 1)
    """

    def __init__(self, in_channels, processing_steps, num_layers=1):
        super(Set2Set, self).__init__()
        self.in_channels = in_channels
        self.out_channels = 2 * in_channels
        self.processing_steps = processing_steps
        self.num_layers = num_layers
        self.lstm = torch.nn.LSTM(self.out_channels, self.in_channels, num_layers)
        self.reset_parameters()

    def reset_parameters(self):
        self.lstm.reset_parameters()

    def forward(self, x, batch):
        batch_size = _ops.num_graphs(batch, x.shape[0])                  # cached: no host read after the first call
        C = self.in_channels
        h = (x.new_zeros((self.num_layers, batch_size, C)), x.new_zeros((self.num_layers, batch_size, C)))
        q_star = x.new_zeros(batch_size, self.out_channels)
        layout = fused_layout(x, batch, batch_size)
        for _ in range(self.processing_steps):
            q, h = self.lstm(q_star.unsqueeze(0), h)
            q = q.view(batch_size, C)
            if layout is not None:
                q_star = _ops.attention_readout(x, layout, q=q, out=x.new_empty(batch_size, 2 * C), col=C)
            else:
                if batch is None:
                    batch = x.new_zeros(x.shape[0], dtype=torch.long)
                e = (x * q[batch]).sum(dim=-1, keepdim=True)
                q_star = torch.cat([q, recipe(x, e, batch, batch_size)], dim=-1)
        return q_star

    def __repr__(self):
        return "{}({}, {})".format(self.__class__.__name__, self.in_channels, self.out_channels)
