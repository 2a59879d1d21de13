// twriter_dev.h -- what a streamed writer with a device path (trim_host.cpp: itsx_twriter_set_device) asks of the context it borrows
// (engine.hip).  Every call takes the context's writer lock for its whole length, so two writers (a paired run's R1 and R2) may share
// one context; after a HIP error every later call on that context returns ITSX_E_DEVICE without touching the device.  `err` names the
// step that failed.
#pragma once
#include <cstdint>
#include <string>
#include "../../include/itsx_hip.h"

namespace itsx {

// the device buffers of a writer whose units hold unit_bytes of text: raw text, line index, records, output text, the deflate scratch
// and the pinned staging buffers -- held from here on, sized for records of 32 bytes or more and --trim-ccs's 68 bytes per record (a unit
// of one long record grows them in mid-run: an allocation that can fail with ITSX_E_DEVICE once the chunk contexts hold the memory)
int twdev_reserve(itsx_ctx *ctx, size_t unit_bytes, std::string &err);

struct TwUnit {
  const char *text; size_t nbytes;              // the unit's raw text (whole records)
  const int32_t *start, *stop; int64_t count;   // its records' coordinates; count as the host counted them
  int mode, ccs;
  const int8_t *strand = nullptr;               // [count], or null where no record of the unit is flipped (itsx_twriter_strands; mode 0)
};
// index, plan, copy and deflate of one unit.  fits = false (and nothing else set): the unit's lines are not 4 per record, or a record is
// malformed -- the caller slices it on the host and hands the text to twdev_text.  comp: the unit's gzip members (empty: no record
// survives); nw / tot: records written and their summed length
int twdev_unit(itsx_ctx *ctx, const TwUnit &u, bool &fits, std::string &comp, int64_t &nw, int64_t &tot, std::string &err);
// the gzip members of a text the host sliced (nbytes > 0)
int twdev_text(itsx_ctx *ctx, const char *text, size_t nbytes, std::string &comp, std::string &err);

}  // namespace itsx
