/* endossl_aug_plan.h -- the per-image plans of the device input path, shared by libendossl_host.so (which
 * writes them: esh_fixmatch_device_plan, esh_comatch_device_plan, esh_labeled_device_plan and the
 * *_from_draws builders) and libendossl_hip.so (whose kernels read them: es_aug_fixmatch_u8, es_aug_strong_u8,
 * es_aug_comatch_u8, es_aug_labeled_u8, es_aug_jitter_u8).  Both libraries report the size of each entry
 * (esh_aug_entry_size / es_aug_entry_size, ..._comatch_entry_size, ..._labeled_entry_size) and
 * endossl/host_aug.py refuses to load when any of them differ.
 *
 * Every parameter that takes double-precision math (op magnitudes, the rotation matrices, the Cutout centre,
 * the resize coefficients, the jitter factors, the hue shift) is resolved on the host.  The device does integer
 * and fp32 pixel work, with two exceptions that depend on the pixels themselves: the histogram-derived values
 * (autocontrast's LUT, Contrast's mean gray) and ColorJitter's hue, whose HSV round trip is per-pixel
 * double-precision work on the device, expression by expression the host's. */
#ifndef ENDOSSL_AUG_PLAN_H
#define ENDOSSL_AUG_PLAN_H
#include <stdint.h>

/* One RandAugmentMC slot.  op / applied are the draws as made; kind is what the device runs: the pool
 * index of op (fixmatch_augment_pool() order), or ES_AUG_NONE when the slot changes nothing (not applied,
 * Identity, a rotation by 0), or ES_AUG_SHIFT for an affine map without cross terms (TranslateX / Y, a
 * zero shear), which Pillow runs as an integer shift. */
enum { ES_AUG_NONE = 5 /* Identity's pool index */, ES_AUG_SHIFT = 14 };

typedef struct EsAugOp {
  int32_t op;       /* pool index drawn, 0..13 */
  int32_t v;        /* magnitude drawn, 1..9 (0..10 from explicit draws) */
  int32_t applied;  /* the slot's apply draw */
  int32_t neg;      /* the slot's sign draw (0 when not applied: it is not made then) */
  int32_t kind;     /* what the device runs (above) */
  float alpha;      /* Brightness / Color / Contrast / Sharpness: the Image.blend factor */
  int32_t mask;     /* Posterize: byte mask */
  int32_t thresh;   /* Solarize: threshold */
  int32_t a[6];     /* Rotate / ShearX / ShearY: 16.16 fixed point a0..a5, a2 and a5 at the first pixel centre */
  int32_t shift_x;  /* ES_AUG_SHIFT: out(x, y) = in(x + shift_x, y + shift_y), black outside */
  int32_t shift_y;
} EsAugOp;

typedef struct EsAugEntry {
  int64_t frame_off;  /* byte offset of the decoded RGB HWC frame in the arena */
  int32_t w, h;       /* frame size */
  int32_t coef_h;     /* int32 offset of the horizontal table (w -> R) in the coefficient buffer; -1: w == R */
  int32_t ksize_h;
  int32_t coef_v;     /* the vertical table (h -> R); -1: h == R */
  int32_t ksize_v;
  int32_t crop;       /* CenterCrop offset into the R x R image (top == left), 0 without IS_CROP */
  int32_t flip;       /* RandomHorizontalFlip draw */
  int32_t top, left;  /* RandomCrop offset into the reflect-padded image */
  EsAugOp ops[2];
  int32_t rect[4];    /* Cutout: x0, y0, x1, y1 as drawn (inclusive corners; the device clips them) */
} EsAugEntry;

/* A table for (in -> out): bounds [out][2] (first input index, count), then kk [out][ksize], all int32. */

/* The frame / resize head every entry begins with (EsAugEntry's first nine fields): the resize kernels read
 * any entry array through it, at the array's own stride. */
typedef struct EsAugHead {
  int64_t frame_off;
  int32_t w, h;
  int32_t coef_h, ksize_h, coef_v, ksize_v;
  int32_t crop;
} EsAugHead;

/* The strong chain's fields, laid out as EsAugEntry's from `flip` to its end, so one kernel reads both. */
typedef struct EsAugStrong {
  int32_t flip;
  int32_t top, left;
  EsAugOp ops[2];
  int32_t rect[4];
} EsAugStrong;

/* A ColorJitter chain on the S x S image, then RandomGrayscale and RandomHorizontalFlip: TransformCoMatch's
 * strong_1 (four ops) and the labeled transform's tail (three ops, never gray or flipped).  order / factor /
 * hue are the draws; kind is what the device runs at each position. */
enum { ES_JIT_BRIGHTNESS = 0, ES_JIT_CONTRAST = 1, ES_JIT_SATURATION = 2, ES_JIT_HUE = 3, ES_JIT_NONE = 4 };

typedef struct EsAugJitter {
  int32_t applied;   /* the RandomApply draw (1 for the labeled transform: its jitter always runs) */
  int32_t nops;      /* positions in use: 4 (with hue) or 3 */
  int32_t order[4];  /* the Fisher-Yates result: ES_JIT_* per position */
  float factor[3];   /* brightness, contrast, saturation: the Image.blend factors, as the host's floats */
  int32_t hue;       /* the hue shift (int)(hue_factor * 255.0), added to H modulo 256 */
  int32_t gray;      /* the RandomGrayscale draw */
  int32_t flip;      /* the RandomHorizontalFlip draw */
  int32_t kind[4];   /* order[k], or ES_JIT_NONE: not applied, past nops, or a blend factor of exactly 1 */
} EsAugJitter;

/* TransformCoMatch: weak = base flipped by flip_w; strong_0 = the strong chain of base under s0 (top == left ==
 * the reflect pad: the crop window is the image itself); strong_1 = the jitter chain of base. */
typedef struct EsAugCoEntry {
  EsAugHead head;
  int32_t flip_w;
  EsAugStrong s0;
  EsAugJitter jit;
} EsAugCoEntry;

/* The labeled train transform: Resize(R) -> h / v flip -> rotation on the R x R image -> CenterCrop(S) at
 * head.crop -> the jitter chain.  rot 0: no rotation (the reduced angle is 0, or its matrix is the identity
 * after Pillow's 15-digit rounding); 1: a[] walks the rotated image as Pillow's 16.16 affine does. */
typedef struct EsAugLabEntry {
  EsAugHead head;
  int32_t hflip, vflip;
  int32_t rot;
  int32_t reserved;
  double angle;  /* the draw, uniform(-20, 20) degrees */
  int32_t a[6];
  EsAugJitter jit;
} EsAugLabEntry;

#endif /* ENDOSSL_AUG_PLAN_H */
