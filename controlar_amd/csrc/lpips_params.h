// lpips_params.h — parameter blocks shared by lpips.hip (kernels) and engine_lpips.hip (host side of car_lpips / car_psnr / car_recon_to_u8).
#pragma once

#define LP_LAYERS 5
#define LP_PASSES 32           // pixel passes of one head workgroup: it owns LP_PASSES * (2048 / C) = 65536 / C consecutive pixels of one pair

// how car_psnr reads an element before the fp64 difference, each step rounded to fp32 once
enum { LP_MAP_RAW = 0, LP_MAP_DIV255 = 1, LP_MAP_HALF = 2 };      // v | v / 255 (the script's sample.astype(float32) / 255.) | (v + 1) / 2 (its rgb_gt)

// The LPIPS head of one tap (lpips.py:89-92,158-164) over the pairs of one chunk.  Image 2i is `a` of pair i, image 2i + 1 its `b`: NHWC maps of P pixels and
// C channels in the element type, img elements apart.  part[(pair * nblk + blk)] = fp64 sum over the workgroup's pixels of sum_c w_c (a_c/(|a|+eps) - b_c/(|b|+eps))^2.
struct LpipsHeadP {
    const void* act; long img;
    const float* lin;              // [C] fp32
    double* part; int nblk;
    long P; int C;
};

// Fold of one chunk: per pair and layer the partials in index order, / P_l, then the layers in the order 0..4.
struct LpipsFoldP {
    const double* part[LP_LAYERS]; int nblk[LP_LAYERS]; double count[LP_LAYERS];
    double* out; double* layers;   // [npairs], [npairs][5] or NULL
    int npairs;
};
