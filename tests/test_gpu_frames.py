"""The camera-frame front on the GPU: ``mvdet_amd.frames.resize_normalize`` against the restatement of the reference's
``T.Compose([T.Resize, T.ToTensor, normalize])`` (``frames_ref``: Pillow's two fixed-point passes, then the torch-CPU
op chain).  The arithmetic is integer and the value table is those very ops, so every comparison is ``torch.equal``.

The kernel's output tiles are 16 x 64, 8 x 64 and 8 x 32 (``frames.TILES``, chosen by the scale): the "tile" cases
straddle them, and one case per tile size runs."""
import numpy as np
import pytest
import torch

import frames_ref as fr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(frames_np, size, **kw):
    from mvdet_amd import frames
    return frames.resize_normalize(torch.from_numpy(np.ascontiguousarray(frames_np)).to(DEV), size, **kw)


# (input, output, B, N): down (2.3x / 2.2x); up; one axis unchanged; identity; 4.4x down on one axis and up on the
# other; an output that is no multiple of any tile in either axis (33 = 2 x 16 + 1 = 4 x 8 + 1, 70 = 64 + 6 =
# 2 x 32 + 6); the 8 x 64 tile (4x down); the 8 x 32 tile (6x down)
SHAPES = [((37, 53), (16, 24), 2, 3), ((16, 24), (37, 53), 1, 2), ((23, 41), (23, 17), 1, 2), ((9, 11), (9, 11), 2, 1),
          ((31, 17), (7, 40), 1, 2), ((70, 131), (33, 70), 2, 2), ((96, 400), (24, 100), 1, 1),
          ((120, 480), (20, 80), 1, 2)]


@pytest.mark.parametrize("in_hw,out_hw,B,N", SHAPES, ids=[f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}" for s in SHAPES])
def test_random_frames_match_the_restatement(in_hw, out_hw, B, N):
    from mvdet_amd import frames
    x = fr.random_frames((B, N, *in_hw, 3), seed=in_hw[1])
    want = fr.transform(x, out_hw)
    got = _run(x, out_hw)
    assert got.shape == (B, N, 3, *out_hw) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), want)
    assert torch.equal(_run(x, out_hw, channels_last=False).cpu(), want)
    tiles = {((96, 400), (24, 100)): (8, 64), ((120, 480), (20, 80)): (8, 32)}
    assert frames.pick_tile(in_hw, out_hw) == tiles.get((in_hw, out_hw), (16, 64))


def test_the_pillow_golden():
    g = fr.golden()
    got = _run(g["random_in"][None, None], (36, 64))
    assert torch.equal(got.cpu()[0, 0], fr.to_tensor_normalize(g["random_out"], fr.MEAN, fr.STD))
    got = _run(g["rows_in"][None, None], (23, 17))
    assert torch.equal(got.cpu()[0, 0], fr.to_tensor_normalize(g["rows_out"], fr.MEAN, fr.STD))


@pytest.mark.parametrize("in_hw,out_hw", [((37, 53), (16, 24)), ((16, 24), (37, 53)), ((70, 131), (33, 70))])
def test_constant_and_alternating_frames(in_hw, out_hw):
    """All 255 must give exactly ``lut[c][255]`` everywhere (the rounding and the clamp: the coefficients of a row
    need not sum to 1 << 22), all 0 exactly ``lut[c][0]``; 0 / 255 stripes are the largest steps the passes see."""
    from mvdet_amd import frames
    lut = frames.value_table().to(DEV)
    H, W = in_hw
    for value in (255, 0):
        got = _run(np.full((1, 2, H, W, 3), value, dtype=np.uint8), out_hw)
        assert torch.equal(got, lut[:, value].view(1, 1, 3, 1, 1).expand_as(got)), value
    stripes = np.stack([fr.alternating(H, W, rows=True), fr.alternating(H, W, rows=False)])[None]
    assert torch.equal(_run(stripes, out_hw).cpu(), fr.transform(stripes, out_hw))


@pytest.mark.parametrize("N", [1, 16])
def test_view_counts(N):
    x = fr.random_frames((1, N, 20, 33, 3), seed=N)
    assert torch.equal(_run(x, (13, 22)).cpu(), fr.transform(x, (13, 22)))


def test_a_list_of_separate_tensors():
    from mvdet_amd import frames
    x = fr.random_frames((2, 3, 37, 53, 3), seed=1)
    want = fr.transform(x, (16, 24))
    views = [torch.from_numpy(x[:, v].copy()).to(DEV) for v in range(3)]
    assert torch.equal(frames.resize_normalize(views, (16, 24)).cpu(), want)
    # views that are not pixel-contiguous (channel-planar storage) are copied, not misread
    planar = [v.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1) for v in views]
    assert not planar[0].is_contiguous()
    assert torch.equal(frames.resize_normalize(planar, (16, 24)).cpu(), want)


def test_a_slice_of_a_wider_buffer_is_read_in_place():
    """A [B,N,H,W,3] window of a wider buffer whose row stride (3 x 59 = 177 bytes) is no multiple of 4, starting at
    an odd byte: read through the strides, and the 255s around the window must not leak in."""
    from mvdet_amd import frames
    B, N, H, W = 2, 2, 37, 53
    x = fr.random_frames((B, N, H, W, 3), seed=2)
    x[:, :, 0], x[:, :, -1], x[:, :, :, 0], x[:, :, :, -1] = 0, 0, 0, 0  # a dark rim: a leaked 255 would show
    wide = torch.full((B, N, H + 4, 59, 3), 255, dtype=torch.uint8)
    wide[:, :, 2:2 + H, 5:5 + W] = torch.from_numpy(x)
    dev_wide = wide.to(DEV)
    window = dev_wide[:, :, 2:2 + H, 5:5 + W]
    assert window.stride(2) == 177 and window.storage_offset() % 4 != 0 and not window.is_contiguous()
    assert frames._in_place(window[:, 0]).data_ptr() == window[:, 0].data_ptr()  # no copy is made
    want = fr.transform(x, (16, 24))
    assert torch.equal(frames.resize_normalize(window, (16, 24)).cpu(), want)
    assert torch.equal(frames.resize_normalize(window[::2], (16, 24)).cpu(), want[::2])  # a batch stride of its own
    assert torch.equal(dev_wide.cpu(), wide), "the source was written"


def test_layouts_and_out():
    from mvdet_amd import frames
    x = fr.random_frames((2, 3, 70, 131, 3), seed=3)
    size = (33, 70)
    want = fr.transform(x, size)
    xd = torch.from_numpy(x).to(DEV)
    cl = frames.resize_normalize(xd, size)
    nchw = frames.resize_normalize(xd, size, channels_last=False)
    assert torch.equal(cl, nchw) and torch.equal(cl.cpu(), want)
    for v in range(3):
        assert cl[:, v].is_contiguous(memory_format=torch.channels_last)
        assert cl[:, v].contiguous(memory_format=torch.channels_last).data_ptr() == cl[:, v].data_ptr()
        assert nchw[:, v].is_contiguous()
    # out= : a window of a larger tensor; its neighbours keep their values
    big = torch.full((2, 5, 3, 35, 75), -7.0, device=DEV)
    window = big[:, 1:4, :, 1:34, 2:72]
    assert frames.resize_normalize(xd, size, out=window) is window
    assert torch.equal(window.cpu(), want)
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[:, 1:4, :, 1:34, 2:72] = False
    assert bool((big[mask] == -7.0).all())
    # 16-byte aligned windows take the float4 stores, here with a last group of columns that is cut (70 = 64 + 4 + 2)
    big = torch.full((2, 5, 3, 36, 76), -7.0, device=DEV)
    big_cl = torch.full((5, 2, 36, 76, 3), -7.0, device=DEV).permute(1, 0, 4, 2, 3)
    for t in (big, big_cl):
        window = t[:, 1:4, :, 1:34, 4:74]
        assert window.data_ptr() % 16 == 0
        frames.resize_normalize(xd, size, out=window)
        assert torch.equal(window.cpu(), want)
        mask = torch.ones_like(t, dtype=torch.bool)
        mask[:, 1:4, :, 1:34, 4:74] = False
        assert bool((t[mask] == -7.0).all())
    # non-default mean / std, and the callable
    mean, std = (0.1, 0.5, 0.9), (0.3, 1.0, 2.5)
    ft = frames.FrameTransform(size, mean, std)
    assert torch.equal(ft(xd).cpu(), fr.transform(x, size, mean, std))


def test_full_size_view():
    """One 1080 x 1920 -> 720 x 1280 view of full-range random bytes (the Wildtrack frame: 45 x 20 tiles)."""
    x = fr.random_frames((1, 1, 1080, 1920, 3), seed=4)
    assert torch.equal(_run(x, (720, 1280)).cpu(), fr.transform(x, (720, 1280)))


@pytest.fixture
def deterministic_backbone():
    """The stock backbone's convolutions in the conv library's deterministic mode: without it two forwards of one
    module on the SAME fp32 input differ in the last bits (measured on the MI355X: 2e-5 on the backbone's maps, 3e-6
    on ``map_result``; exactly 0 with it), so no bitwise comparison of two forwards could hold."""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = before


@pytest.mark.parametrize("cls_name", ["PerspTransDetector", "NoJointConvVariant", "ImageProjVariant"])
def test_modules_take_decoded_frames(cls_name, deterministic_backbone):
    """``Module(ds, frame_transform=ft)(u8)`` is bitwise the same module on ``ft(u8)``; a float input takes the old
    path; the ``state_dict`` does not know the transform."""
    import mvdet_amd
    from mvdet_amd import FrameTransform, synthetic
    ds = synthetic.wildtrack_like(2, 4, seed=0, img_shape=(108, 192), worldgrid_shape=(96, 288))
    ft = FrameTransform((108, 192))
    torch.manual_seed(0)
    model = getattr(mvdet_amd, cls_name)(ds, device=DEV, frame_transform=ft).eval()
    u8 = torch.from_numpy(fr.random_frames((1, 2, 162, 288, 3), seed=5)).to(DEV)
    with torch.no_grad():
        x = ft(u8)
        assert torch.equal(x.cpu(), fr.transform(u8.cpu().numpy(), (108, 192)))
        model(x)  # (a module's first forward builds its workspaces and lets the conv library pick its algorithms)
        map_u8, imgs_u8 = model(u8)
        map_f, imgs_f = model(x)             # a float input: the old path
        map_host, _ = model(u8.cpu())        # decoded frames still on the host are moved first
        model.frame_transform = None
        map_plain, imgs_plain = model(x)     # the module without a transform
    print("max |d map|:", [float((map_u8 - m).abs().max()) for m in (map_f, map_plain, map_host)])
    assert torch.equal(map_u8, map_f) and torch.equal(map_u8, map_plain) and torch.equal(map_u8, map_host)
    assert len(imgs_u8) == len(imgs_f) == 2
    for a, b, c in zip(imgs_u8, imgs_f, imgs_plain):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.isfinite(map_u8).all()
    assert not any("frame" in k for k in model.state_dict())
