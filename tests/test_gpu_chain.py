"""The gradient chain on the GPU: ``ops.chain.GradChain`` (what the attack and attribution loops launch) against
``Predictor.input_gradient`` (the two autograd Functions), bit for bit."""
import pytest
import torch

from pytorch_mnist_ddp_amd.data.datasets import normalize_u8
from pytorch_mnist_ddp_amd.data.synthetic import generate
from pytorch_mnist_ddp_amd.inference import Predictor
from pytorch_mnist_ddp_amd.models.net import Net
from pytorch_mnist_ddp_amd.ops.chain import GradChain
from pytorch_mnist_ddp_amd.ops.fused_net import fused_state

pytestmark = pytest.mark.gpu


# rows = 1: below one 32-row head tile; 33: above it (Bp = 64), on an activation set of more rows than the launch
@pytest.mark.parametrize("rows", [1, 33])
def test_grad_chain_equals_predictor_input_gradient(cuda_device, rows):
    dev = cuda_device
    torch.manual_seed(3)
    net = Net().to(dev).train()
    pr = Predictor(net)
    imgs, labels = generate(rows, seed=5)
    x = normalize_u8(imgs).reshape(rows, 784).to(dev).contiguous()
    want, _ = pr.input_gradient(x.view(rows, 1, 28, 28), labels.to(dev))
    assert torch.isfinite(want).all() and want.any()
    st = fused_state(net)
    st.sync()
    offset, pooled = st.rng_offset, sum(len(v) for v in st.pool.values())
    lab = labels.to(dev, torch.int32).contiguous()
    dx = torch.full((rows, 784), float("nan"), device=dev)
    chain = GradChain(st, rows + 7)
    chain.run(x.data_ptr(), lab.data_ptr(), rows)
    chain.input_grad(dx.data_ptr(), rows)
    chain.release()
    assert torch.equal(dx.view(rows, 1, 28, 28), want)
    assert st.rng_offset == offset and sum(len(v) for v in st.pool.values()) == pooled + 1
