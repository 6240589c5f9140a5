"""The entry points of the fused CNN kernels that no other GPU test drives through their masked re-run, or compares bit for bit with a
second entry point (profiles/cnn_host_refactor.md lists which test covers each of the others): buf_cylindrical_net_split_safe (the form
left to the library) against buf_cylindrical_net_wg, buf_cylindrical_net_split_safe_all against buf_cylindrical_net_wg_all, and
buf_cost_volume_net_split_safe, dense and gathered, against buf_cost_volume_net / buf_cost_volume_net_gather.

Three patches / matches, the middle one scaled by 1e6: the smallest batch with a flagged workgroup between two that return at once.  The
flagged row must be the plain fp32 entry point's bit for bit, the other two the split kernel's own."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def W():
    from buffer_amd.weights import load_weights
    return load_weights('3dmatch')


@pytest.fixture(scope='module')
def layers(W, dev):
    from buffer_amd.config import THREEDMATCH
    from buffer_amd.patch_embedder import PatchEmbedder
    return PatchEmbedder(W, dev, THREEDMATCH).layers


@pytest.fixture(scope='module')
def patches(dev):
    g = torch.Generator(device='cpu').manual_seed(5)
    x = torch.rand((3, 48, 140), generator=g).to(dev)
    bad = x.clone()
    bad[1] *= 1e6
    return x, bad


def bits(t):
    return t.view(torch.int32)


def only_the_middle_one_rerun(flags, got, clean, want):
    assert (flags != 0).tolist() == [False, True, False]
    assert torch.equal(bits(got[1]), bits(want[1]))
    assert torch.equal(bits(got[0]), bits(clean[0])) and torch.equal(bits(got[2]), bits(clean[2]))


def test_split_safe_with_the_form_left_to_the_library(layers, patches, dev):
    from buffer_amd import _lib, ops
    from buffer_amd.ops import _ptr, _stream
    x, bad = patches
    split = ops.CylindricalNetSplit(layers, dev, f24p=True)            # the pass-split form: what the library's default means
    net, L = split.f32, _lib.lib()
    assert split.safe and split.fn == "buf_cylindrical_net_split_safe_form" and net.fn == "buf_cylindrical_net_wg_form" and net.form == 1

    def safe(t):
        y, flags = torch.empty((3, 32, 7, 20), device=dev), torch.empty((3,), dtype=torch.int32, device=dev)
        ops.check(L.buf_cylindrical_net_split_safe(_ptr(t), 3, split._wp, split._wwp, split._bp, split._ci, split._co, split._re_safe, None, _ptr(y),
                                                   None, _ptr(split.status), _ptr(flags), _stream()), "buf_cylindrical_net_split_safe")
        return y, flags

    def plain(t):
        y = torch.empty((3, 32, 7, 20), device=dev)
        ops.check(L.buf_cylindrical_net_wg(_ptr(t), 3, net._wp, net._bp, net._ci, net._co, net._re, _ptr(y), _stream()), "buf_cylindrical_net_wg")
        return y

    clean, none = safe(x)
    assert not bool(none.any())
    got, flags = safe(bad)
    want = plain(bad)
    only_the_middle_one_rerun(flags, got, clean, want)
    assert torch.equal(bits(want), bits(net(bad)))                     # buf_cylindrical_net_wg is buf_cylindrical_net_wg_form at that form
    assert torch.equal(bits(got), bits(split(bad)))                    # and likewise for the split-safe pair


def test_split_safe_all(layers, patches, dev):
    from buffer_amd import ops
    x, bad = patches
    split, net = ops.CylindricalNetSplit(layers, dev, f24a='all', f25='off'), ops.CylindricalNet(layers, dev, f24a='all', f25='off')
    assert split.safe and split.fn == "buf_cylindrical_net_split_safe_all" and net.fn == "buf_cylindrical_net_wg_all" and split.f24_all
    clean = split(x)
    assert split.range_fallbacks() == 0
    got = split(bad)
    only_the_middle_one_rerun(split.last_flags, got, clean, net(bad))


def test_cost_split_safe_dense_and_gathered(W, dev):
    from buffer_amd import registration
    cvs, cv32 = registration.CostVolume(W, dev, arith='split', f24='off').fused, registration.CostVolume(W, dev, f24='off').fused
    assert cvs.safe and cvs.f32.kernel == "" and cv32.kernel == ""     # the entry points without sets
    g = torch.Generator(device='cpu').manual_seed(6)
    equi = F.normalize(torch.rand((6, 32, 7, 20), generator=g), dim=1).to(dev)
    s_rows, t_rows = torch.arange(0, 3, device=dev), torch.arange(3, 6, device=dev)
    bad = equi.clone()
    bad[1] *= 1e6                                                      # the source map of match 1 only
    dense = lambda e: (e[s_rows][:, :, 1:6].contiguous(), e[t_rows][:, :, 1:6].contiguous())
    clean = cvs(*dense(equi))
    assert cvs.range_fallbacks() == 0
    want = cv32(*dense(bad))
    got = cvs(*dense(bad))
    only_the_middle_one_rerun(cvs.last_flags, got, clean, want)
    assert torch.equal(bits(cv32.gathered(bad, s_rows, t_rows)), bits(want))            # buf_cost_volume_net_gather is buf_cost_volume_net, gather fused
    clean_g = cvs.gathered(equi, s_rows, t_rows)
    got_g = cvs.gathered(bad, s_rows, t_rows)
    only_the_middle_one_rerun(cvs.last_flags, got_g, clean_g, want)
