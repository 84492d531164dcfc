"""Numpy restatement of the loader's pooling conversion (wfae_vil_pool_u8_to_f32, include/wfae.h): every ft-th frame of a
uint8 'NHWT' batch, then a max (the offline sevir_lr recipe: ceil sizes, a block at the edge reduced over its pixels inside)
or a mean (the runtime downsample_data_dict: floor sizes, remainder dropped) over fh x fw blocks, as fp32 'NTHW'.

    v(b)  = scale * (float32(b) + offset)                  one add, then one multiply, each rounded to fp32
    max:  v(max of the block's bytes)
    mean: acc = 0; for a in range(fh): for b in range(fw): acc = acc + v(byte[a][b]);  acc / float32(fh * fw)

max + augmentation is `augment_ref.augment_batch(pool_max_u8(u8, f), params)`: the transform acts on the pooled grid.
"""
import numpy as np

SCALE_01, OFFSET_01 = 1 / 255, 0.0
SCALE_SEVIR, OFFSET_SEVIR = 1 / 47.54, -33.44


def pool_max_u8(u8_nhwt, f):
    """uint8 (N, H, W, T) -> uint8 (N, ceil(H/fh), ceil(W/fw), ceil(T/ft))"""
    ft, fh, fw = f
    x = u8_nhwt[..., ::ft]
    N, H, W, T = x.shape
    Ho, Wo = -(-H // fh), -(-W // fw)
    pad = np.zeros((N, Ho * fh, Wo * fw, T), np.uint8)           # block_reduce pads with 0: neutral for a max over uint8
    pad[:, :H, :W] = x
    return pad.reshape(N, Ho, fh, Wo, fw, T).max(axis=(2, 4))


def value(u8, scale, offset):
    return np.float32(scale) * (u8.astype(np.float32) + np.float32(offset))


def pool(u8_nhwt, f, mode, scale=SCALE_01, offset=OFFSET_01):
    """uint8 (N, H, W, T) -> fp32 (N, To, Ho, Wo)"""
    ft, fh, fw = f
    if mode == "max":
        return np.ascontiguousarray(value(pool_max_u8(u8_nhwt, f), scale, offset).transpose(0, 3, 1, 2))
    assert mode == "mean"
    x = u8_nhwt[..., ::ft]
    N, H, W, T = x.shape
    Ho, Wo = H // fh, W // fw
    v = value(x[:, :Ho * fh, :Wo * fw], scale, offset).reshape(N, Ho, fh, Wo, fw, T)
    acc = np.zeros((N, Ho, Wo, T), np.float32)
    for a in range(fh):                                          # block row-major order, one rounded add at a time
        for b in range(fw):
            acc = acc + v[:, :, a, :, b]
    out = acc / np.float32(fh * fw)
    assert out.dtype == np.float32
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2))
