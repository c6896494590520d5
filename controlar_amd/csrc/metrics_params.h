// metrics_params.h — parameter blocks shared by metrics.hip (kernels) and engine_metrics.hip (host side of car_ms_ssim / car_f1 / car_rmse / car_pixels_to_u8).
#pragma once

enum { MT_F32 = 0, MT_U8 = 4 };                  // element types of a metric input: the CAR_DT_* codes
enum { MT_RULE_EQ = 0, MT_RULE_GT = 1 };         // car_f1: what counts as positive, v == value or v > value

#define MS_T 32            // output tile side
#define MS_K 11            // window side
#define MS_HALO (MS_T + MS_K - 1)
#define MS_STRIP 16        // output rows column-filtered per pass over the row-filtered maps
#define MS_SCALES 5
#define MS_C1 1e-4         // (0.01 * data_range)^2, data_range = 1
#define MS_C2 9e-4         // (0.03 * data_range)^2

struct MsScaleP {
    const void* p; const void* t; int dt_p, dt_t;   // [planes, H, W] fp32 or uint8
    double scale_p, scale_t;                        // value = clip(v * scale, 0, 1)
    int H, W, tiles_x, tiles_y;                     // tiles over the (H - 10) x (W - 10) map
    float* next_p; float* next_t; int Hn, Wn;       // avg_pool2d(2) of both images [planes, H/2, W/2], or NULL at the last scale
    double* part;                                   // [planes][tiles_y * tiles_x][2]: sums of ssim and of cs over a tile
    double g[MS_K];                                 // the normalised 1-D Gaussian
};

struct MsFoldP {
    const double* part; long off[MS_SCALES];        // the partials of scale s start at part + off[s]
    int ntile[MS_SCALES]; double count[MS_SCALES];  // tiles per plane; values per image, C (H_s - 10) (W_s - 10)
    double beta[MS_SCALES];
    int C;
    double* out;                                    // [B]
    double* table;                                  // [B][5][2] (ssim, cs) means after relu, or NULL
};
