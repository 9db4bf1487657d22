// The row of the tables that describe a frame's ANSWER -- { form, h, w, answer, answer_bytes, K, ids, 0 } (include/frtm_hip.h) -- and its check,
// defined once for the launches that take such a table: the object report (object_report.hip) and the run-length coder (mask_runs.hip).  A
// table built for one call serves the other.
#pragma once
#include "frtm_common.h"
#include "per_frame.h"       // MERGE_MAX
#include "../../include/frtm_hip.h"

#define OB_MAXDIM 16384
#define OB_MAXBYTES (1LL << 46)
#define OB_ROW FRTM_OBJECT_ROW_WORDS
#define OB_SLOTS FRTM_OBJECT_SLOTS
#define OB_NONE 255         // slot of a label-map pixel whose id is not listed

static_assert(OB_SLOTS == MERGE_MAX, "a slot per plane of a merged stack");

// words of a table row
enum { OW_FORM, OW_H, OW_W, OW_ANS, OW_ANS_BYTES, OW_K, OW_IDS, OW_ZERO };
// why a row is refused
enum { OB_OK, OB_BAD_ENUM, OB_BAD_SIZE, OB_BAD_K, OB_NULL, OB_NOT_A_SIZE, OB_ANS_RANGE, OB_ANS_ALIGN };

// Is row r a frame this launch can read?  (Evaluated by the host from its copy, for the messages and the grid, and by every workgroup from
// the DEVICE table before it touches anything: a device table that differs from the checked one reads nothing out of bounds.)
__host__ __device__ static inline int ob_check(const long long* r) {
  const long long form = r[OW_FORM], h = r[OW_H], w = r[OW_W], K = r[OW_K], ab = r[OW_ANS_BYTES];
  if ((form != FRTM_OBJECT_LABELS && form != FRTM_OBJECT_MASKS) || r[OW_ZERO] != 0) return OB_BAD_ENUM;
  if (h < 1 || w < 1 || h > OB_MAXDIM || w > OB_MAXDIM) return OB_BAD_SIZE;
  if (K < 1 || K > OB_SLOTS) return OB_BAD_K;
  if (!r[OW_ANS] || !r[OW_IDS]) return OB_NULL;
  if (ab < 0 || ab > OB_MAXBYTES) return OB_NOT_A_SIZE;
  if ((form == FRTM_OBJECT_MASKS ? 4 * K * h * w : h * w) > ab) return OB_ANS_RANGE;
  if (form == FRTM_OBJECT_MASKS && (r[OW_ANS] & 3)) return OB_ANS_ALIGN;
  return OB_OK;
}

// The host's pass over its copy of the table: FRTM_OK, or FRTM_ERR_ARG with the message that names the first refused frame.
static inline int ob_check_table(const char* who, const long long* table_host, int n) {
  for (int i = 0; i < n; ++i) {
    const long long* r = table_host + (size_t)OB_ROW * i;
    switch (ob_check(r)) {
      case OB_OK: break;
      case OB_BAD_ENUM:
        FRTM_CHECK_ARG(false, "%s: frame %d has answer form %lld and last word %lld (a form of include/frtm_hip.h, and 0)", who, i, r[OW_FORM], r[OW_ZERO]);
      case OB_BAD_SIZE: FRTM_CHECK_ARG(false, "%s: frame %d has size %lld x %lld (1 .. %d)", who, i, r[OW_H], r[OW_W], OB_MAXDIM);
      case OB_BAD_K: FRTM_CHECK_ARG(false, "%s: frame %d has K = %lld slots (1 .. %d)", who, i, r[OW_K], OB_SLOTS);
      case OB_NULL: FRTM_CHECK_ARG(false, "%s: frame %d has a null address (answer %#llx, ids %#llx)", who, i, r[OW_ANS], r[OW_IDS]);
      case OB_NOT_A_SIZE: FRTM_CHECK_ARG(false, "%s: frame %d: answer_bytes %lld is not a size", who, i, r[OW_ANS_BYTES]);
      case OB_ANS_RANGE:
        FRTM_CHECK_ARG(false, "%s: frame %d's answer (%lld bytes) leaves its %lld-byte buffer", who, i,
                       r[OW_FORM] == FRTM_OBJECT_MASKS ? 4 * r[OW_K] * r[OW_H] * r[OW_W] : r[OW_H] * r[OW_W], r[OW_ANS_BYTES]);
      default: FRTM_CHECK_ARG(false, "%s: frame %d's mask stack at %#llx is not 4-byte aligned", who, i, r[OW_ANS]);
    }
  }
  return FRTM_OK;
}
