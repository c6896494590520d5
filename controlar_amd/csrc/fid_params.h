// fid_params.h — constants and launch descriptors shared by fid.hip (kernels) and engine_fid.hip (host side) for the statistics half of
// evaluations/c2i/evaluator.py: the fp64 moments behind FID / sFID, the k-NN manifold of precision / recall, the Inception Score.
#pragma once

#define FID_KMAX 8        // a row keeps its FID_KMAX smallest distances: k + 1 <= FID_KMAX
#define FID_TM 128        // a workgroup's distance tile: FID_TM rows x FID_TN columns
#define FID_TN 64
#define FID_KC 32         // k step of the tile loop: features are padded to a multiple of it with zeros
#define FID_CLD 65        // row stride of the fp32 tile in LDS (odd: row scans and column scans are both conflict-free)
#define FID_COV_T 64      // the covariance kernel's output tile (FID_COV_T x FID_COV_T) ...
#define FID_COV_K 32      // ... and the rows of a batch it stages at a time
#define FID_COV_LD 72     // row stride (doubles) of a staged slab

enum { FID_F16 = 0, FID_F32 = 1 };                                              // the arithmetic of a distance block
enum { FID_EPI_KSMALL = 0, FID_EPI_THRESH = 1, FID_EPI_STORE = 2, FID_EPI_PRODUCT = 3 };

// One launch of the tile loop: rows of U against rows of V.  Workgroup index = (cb * nrb + rb) * rt_per_rb + rt: row tile rt of row batch rb walks the
// columns of column batch cb.  flags [ncb * nrb] (index cb * nrb + rb): the fp16 launch raises a block's flag when one of its distances is not finite;
// the fp32 launch returns at once where the flag is down (NULL: run everywhere).
struct FidTileP {
    const void* U; const void* V;            // FID_F16: the fp16 copies [n][Dp]; FID_F32: the fp32 originals [n][D]
    long ldu, ldv;                           // row strides in elements
    const void* nu; const void* nv;          // squared norms per row in the launch's arithmetic (fp16 bits / fp32); unused by FID_EPI_PRODUCT
    long N1, N2;
    int D, Kp;                               // Kp = D rounded up to FID_KC
    long row_batch, col_batch;
    int rt_per_rb, nrb, ncb;
    int* flags;
    float* lists;                            // KSMALL: [ncb][N1][FID_KMAX], ascending
    const float* r1; const float* r2;        // THRESH: the radii of U's rows / V's rows
    unsigned char* s1part;                   // THRESH: [ncb][N1]               any_j d_ij <= r2[j] over the columns of batch cb
    unsigned char* s2part;                   // THRESH: [nrb * rt_per_rb][N2]   any_i d_ij <= r1[i] over the rows of one row tile
    float* out; long ldo;                    // STORE / PRODUCT: [N1][ldo]
};
