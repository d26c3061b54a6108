/* endossl_aug_plan.h -- the per-image plan of the device input path, shared by libendossl_host.so (which
 * writes it: esh_fixmatch_device_plan, esh_aug_plan_from_draws) and libendossl_hip.so (whose kernels read
 * it: es_aug_fixmatch_u8, es_aug_strong_u8).  Both libraries report sizeof(EsAugEntry)
 * (esh_aug_entry_size / es_aug_entry_size) and endossl/host_aug.py refuses to load when they differ.
 *
 * Every parameter that takes double-precision math (op magnitudes, the rotation matrix, the Cutout centre,
 * the resize coefficients) is resolved on the host; the device does integer and fp32 pixel work only. */
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

#endif /* ENDOSSL_AUG_PLAN_H */
