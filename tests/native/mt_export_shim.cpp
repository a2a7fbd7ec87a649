// C entry points for tests/test_mt_export_cpu.py: the host-side MT19937 export and import of the canonical get_state / set_state
// records, as the env libraries compile them (csrc/cge_host.hpp).  The export returns 0, or -1 when it refuses the stream.
#include "../../custom_gymnasium_environments_amd/csrc/cge_device.hpp"
#include "../../custom_gymnasium_environments_amd/csrc/cge_host.hpp"

extern "C" int mt_export_shim(const uint32_t *w, uint32_t pos, uint32_t pretw, uint32_t *omt, int32_t *idx, const uint32_t *old0) {
    return cge::mt_export_cpython(w, pos, pretw, omt, idx, old0) ? 0 : -1;
}

extern "C" uint32_t mt_export_shim_max_ahead() { return cge::MT_EXPORT_MAX_AHEAD; }

extern "C" uint32_t mt_ready_decode_shim(uint32_t q) { return cge::mt_ready_decode(q); }

extern "C" void mt_import_shim(const uint32_t *words624, int32_t index, uint32_t *block640, uint32_t *pos, uint32_t *pretw) {
    cge::mt_import_cpython(words624, index, block640, pos, pretw);
}

extern "C" int64_t state_chunk_shim() { return cge::STATE_CHUNK; }
