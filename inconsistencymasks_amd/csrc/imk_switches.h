// The environment switches that still change which kernel or launch form runs ("Which kernel runs, and the
// switches that remain").  Each is read once, on first use, by imk_switches(); the dispatch code reads the fields.  Unset = the
// default, which is what the measurements settled on; the other settings are kept for the tests that compare the forms.
#pragma once

struct ImkSwitches {
    bool conv_wide;           // IMK_CONV_WIDE=0: no conv_wide_kernel (17-32 channel layers take the GEMM-class or per-tile kernel)
    bool conv_gemm;           // IMK_CONV_GEMM=0: no GEMM-class kernels, neither the convs' (imk_gemm.hip) nor the weight gradients' (imk_wgemm.hip)
    int conv_chain_tile;      // IMK_CONV_CHAIN_TILE: the per-tile kernel's chain -- 0 off, 1 (default) by the rule of imk_conv_can_chain_tile, 2 always
    bool conv_prestage;       // IMK_CONV_PRESTAGE=0: no 1x1 first stage in front of the pipelined chain (imk_conv_can_prestage)
    bool wide_chain;          // IMK_WIDE_CHAIN=0: no conv_wide_kernel chain
    bool wide_chain_train;    // IMK_WIDE_CHAIN_TRAIN=0: that chain in inference only
    bool gemm_chain;          // IMK_GEMM_CHAIN=0: no GEMM-class chain (imk_conv_gemm_chain_ok)
    int gemm_over_chain;      // IMK_GEMM_OVER_CHAIN: where the GEMM-class kernel takes the 3x3 -- 0 chain anyway, 1 (default) two launches
                              // when the intermediate is stored, 2 always two launches
    int gemm_ad3_wgs;         // IMK_GEMM_AD3_WGS: largest GEMM-class launch (workgroups) of the deep-look-ahead form, 0 never (default 1024)
    int wgrad_gemm_min;       // IMK_WGRAD_GEMM_MIN: channel threshold of the GEMM-class weight gradient for every size (0, default: the rule)
    bool wgrad_nfo2;          // IMK_WGRAD_NFO2=0: no two-output-tile form of the GEMM-class 3x3 weight gradient
    bool student_fused;       // IMK_STUDENT_FUSED=0: imk_unet_forward_student takes forward -> label -> imk_augment for every shape
    bool consistency_fused;   // IMK_CONSISTENCY_FUSED=0: imk_unet_consistency_fwd_bwd takes head_kernel x 2 -> consistency_dlogit_kernel -> the head's dgrad for every shape
    bool dice_fused;          // IMK_DICE_FUSED=0: loss kind 4 takes dice_dlogit_kernel -> the head's dgrad for every shape (no head_mse_fused_kernel variant)
    bool select_shared;       // IMK_SELECT_SHARED=0: imk_evalnet_forward_select scores through imk_evalnet_forward on the repeated images
    int side_streams;         // IMK_SIDE_STREAMS: side streams of a training step's weight gradients, 0 ... MAX_SIDE (default 1)
};

const ImkSwitches &imk_switches();
