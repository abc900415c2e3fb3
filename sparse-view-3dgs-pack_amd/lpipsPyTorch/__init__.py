"""Drop-in for the reference's lpipsPyTorch package: lpips(x, y, net_type='vgg') and LPIPS('vgg') under its names, served by
csrc/gs_lpips.hip (gsplat_amd/lpips.py).  Only net_type='vgg', version '0.1', forward only.  The weights are
gsplat_amd.lpips.set_default_weights(...)'s, else the two files under torch.hub.get_dir()/checkpoints; nothing is fetched."""
import torch

from gsplat_amd import lpips as _impl

__all__ = ["lpips", "LPIPS"]


class LPIPS(torch.nn.Module):
    def __init__(self, net_type: str = 'alex', version: str = '0.1'):
        assert version in ['0.1'], 'v0.1 is only supported now'
        super().__init__()
        if net_type != 'vgg':
            raise NotImplementedError("net_type %r: only 'vgg' is served here (the reference's metrics use nothing else)" % (net_type,))
        self.weights = _impl.default_weights()

    def forward(self, x: torch.Tensor, y: torch.Tensor):
        """-> [1,1,1,1] float32, the float64 result rounded once.  One view per call, as the reference's metrics call it."""
        return _impl.lpips_vgg(x, y, self.weights).to(torch.float32).reshape(1, 1, 1, 1)


def lpips(x: torch.Tensor, y: torch.Tensor, net_type: str = 'alex', version: str = '0.1'):
    return LPIPS(net_type, version)(x, y)
