"""ORACLE support — the small network configurations used by the golden fixtures and parity tests.

They keep every structural feature of the shipped configs (GroupNorm32, two Swin blocks per stage with
a shifted second block, 8x8 windows with 32-channel heads, FiLM ResBlocks, skip concats whose group
boundaries straddle the two sources, VQ-f4 autoencoder with a mid attention block) at a size the CPU
oracle evaluates in well under a second.
"""
TINY_UNET = dict(image_size=16, in_channels=3, model_channels=32, out_channels=3, attention_resolutions=[16, 8], dropout=0,
                 channel_mult=[1, 2], num_res_blocks=[1, 1], conv_resample=True, dims=2, use_fp16=False, num_head_channels=32,
                 use_scale_shift_norm=True, resblock_updown=False, swin_depth=2, swin_embed_dim=64, window_size=8, mlp_ratio=2,
                 cond_lq=True, lq_size=16)
# feature-extractor + mask variant (inpaint / faceir style conditioning, models/unet.py:689-702)
TINY_UNET_FE = dict(TINY_UNET, lq_size=64, cond_mask=True)
TINY_AE = dict(embed_dim=3, n_embed=512,
               ddconfig=dict(double_z=False, z_channels=3, resolution=64, in_channels=3, out_ch=3, ch=32, ch_mult=[1, 2, 4],
                             num_res_blocks=1, attn_resolutions=[], dropout=0.0, padding_mode="zeros"))
TINY_DIFFUSION = dict(sf=4, schedule_name="exponential", schedule_kwargs=dict(power=0.3), etas_end=0.99, steps=4, min_noise_level=0.2,
                      kappa=2.0, weighted_mse=False, predict_type="xstart", timestep_respacing=None, scale_factor=1.0,
                      normalize_input=True, latent_flag=True)
# sf=1 variant used together with TINY_UNET_FE (inpainting-like: lq at image resolution, latent at /4)
TINY_DIFFUSION_SF1 = dict(TINY_DIFFUSION, sf=1)
# faceir-style: 8-channel latent, conditioning through the feature extractor without a mask
TINY_UNET_FE8 = dict(TINY_UNET, in_channels=8, out_channels=8, lq_size=64)
TINY_AE8 = dict(embed_dim=8, n_embed=256,
                ddconfig=dict(double_z=False, z_channels=8, resolution=64, in_channels=3, out_ch=3, ch=32, ch_mult=[1, 2, 4],
                              num_res_blocks=[1, 2, 1], attn_resolutions=[], dropout=0.0, padding_mode="zeros"))

# ---- structures off the two the fixtures above build.  Each entry flips ONE switch of the constructor loops (models/unet.py:704-863,
# ldm/modules/diffusionmodules/model.py:452-660); every key it does not name is TINY_UNET's / TINY_AE's.
def _ae(embed_dim=3, n_embed=512, **dd):
    return dict(embed_dim=embed_dim, n_embed=n_embed, ddconfig=dict(TINY_AE["ddconfig"], **dd))


STRUCTURES = {
    "unet": {
        # no down / upsample at all; Swin layers of a single block: the last one, unshifted
        "one_level": dict(TINY_UNET, channel_mult=[1], num_res_blocks=[2], attention_resolutions=[16], swin_depth=1),
        # a level of ResBlocks without a skip conv (1 -> 1), unequal block counts (skip-stack pops, output_blocks.N.M sub-indices), Swin at
        # the middle level only, an 8 x 8 middle block
        "three_uneven": dict(TINY_UNET, image_size=32, lq_size=32, channel_mult=[1, 1, 2], num_res_blocks=[2, 1, 3], attention_resolutions=[16]),
        # channel_mult[0] != 1: input_ch = 64 feeds the head conv; C = 96 is 3 channels per GroupNorm group; Swin at the coarse level only
        "mult0": dict(TINY_UNET, channel_mult=[2, 3], num_res_blocks=[1, 2], attention_resolutions=[8]),
        # odd depth: shifts 0 / 4 / 0 and a shifted block that is not the last; 3 heads; hidden = int(96 * 1.5) = 144, no multiple of 64
        "depth3": dict(TINY_UNET, image_size=32, lq_size=32, swin_depth=3, swin_embed_dim=96, mlp_ratio=1.5, attention_resolutions=[32, 16]),
        # no level has a Swin layer: the middle block's is the only one
        "no_level_attn": dict(TINY_UNET, attention_resolutions=[]),
        # one feature-extractor stage fed 4 planes (lq | mask); a 4-channel latent next to 32 feature channels at the first conv
        "fe1_mask": dict(TINY_UNET, in_channels=4, out_channels=4, lq_size=32, cond_mask=True),
        # E = 192 / 6 heads / hidden 768 off model_channels 160: the fused attention and the fused MLP WITHOUT the patch-unembed fold, on
        # 128-channel conv tiles.  attention_resolutions is [32, 16], not TINY_UNET's [16, 8]: the fused MLP wants 16384 tokens in a launch,
        # and only a Swin layer at the constructed 32 x 32 level has them at B = 16 (at the 16 x 16 level B = 64 would be needed)
        "heads6_mc128": dict(TINY_UNET, image_size=32, lq_size=32, model_channels=128, swin_embed_dim=192, mlp_ratio=4, channel_mult=[1, 2],
                             attention_resolutions=[32, 16]),
        # the same on 192- and 384-channel layers: the planners' BC = 192 choices and their refusal of it in split storage
        "heads6_mc192": dict(TINY_UNET, image_size=32, lq_size=32, model_channels=192, swin_embed_dim=192, mlp_ratio=4, channel_mult=[1, 2],
                             attention_resolutions=[32, 16]),
    },
    "ae": {
        # one level: no resampling conv in either direction (f = 1)
        "ae_f1": _ae(ch_mult=[1], num_res_blocks=1, resolution=16),
        # equal neighbours in ch_mult: ResNet blocks without nin_shortcut; z_channels != embed_dim; the D = 4 VQ kernel (f = 8)
        "ae_f8_equal": _ae(embed_dim=4, n_embed=256, ch_mult=[1, 1, 2, 2], num_res_blocks=[2, 1, 1, 2], z_channels=8),
        # 192-channel blocks (f = 2)
        "ae_f2_wide": _ae(ch=64, ch_mult=[1, 3]),
    },
    # the whole loop: (unet, autoencoder, sf, mask).  sf and the autoencoder's factor f give the latent: LR * sf / f
    "pairs": {
        "one_level+ae_f1": ("one_level", "ae_f1", 1, False),          # LR 16 x 16, latent 16 x 16, no feature extractor
        "fe1_mask+ae_f8_equal": ("fe1_mask", "ae_f8_equal", 4, True),  # LR 32 x 32 with a mask, image 128 x 128, latent 16 x 16
    },
}


def structure_pair(tag):
    """(unet params, autoencoder params, diffusion params, with_mask) of a STRUCTURES pair"""
    u, a, sf, with_mask = STRUCTURES["pairs"][tag]
    return STRUCTURES["unet"][u], STRUCTURES["ae"][a], dict(TINY_DIFFUSION, sf=sf), with_mask
