// A stand-alone host of csrc/step_table.h's load records (no HIP, no
// libmpcr): reads packed model blobs (mpcr_model_t, .mpcrm), builds each one's
// step table and load records and writes them to <blob>.rec as four int32
// sizes (records, pair set-up record, equality record, pair quad 3) followed
// by the raw StepTable and the raw StepRecords.  Built with the address and
// undefined-behaviour sanitizers and run by tests/test_step_records.py.
//   step_records_host <model.mpcrm>...
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../manipulator_mujoco_amd/csrc/step_table.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  for (int a = 1; a < argc; a++) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 3; }
    std::vector<mpcr_model_t> m(1);
    const size_t got = fread(m.data(), 1, sizeof(mpcr_model_t), f);
    fclose(f);
    if (got != sizeof(mpcr_model_t) || m[0].magic != MPCR_MODEL_MAGIC || m[0].version != MPCR_MODEL_VERSION) {
      fprintf(stderr, "%s is not a v%d model blob\n", argv[a], MPCR_MODEL_VERSION);
      return 4;
    }
    std::vector<mpcr::StepTable> t(1);
    std::vector<mpcr::StepRecords> r(1);
    if (mpcr::build_step_table(m[0], t[0]) != 0 || mpcr::build_step_records(m[0], r[0]) != 0) {
      fprintf(stderr, "%s exceeds the table\n", argv[a]);
      return 5;
    }
    const int32_t sizes[4] = {(int32_t)sizeof(mpcr::StepRecords), (int32_t)sizeof(mpcr::StepPairSetup),
                              (int32_t)sizeof(mpcr::StepEq), (int32_t)sizeof(mpcr::StepPairJ)};
    const std::string out = std::string(argv[a]) + ".rec";
    FILE* o = fopen(out.c_str(), "wb");
    if (!o || fwrite(sizes, sizeof(sizes), 1, o) != 1 || fwrite(t.data(), sizeof(mpcr::StepTable), 1, o) != 1 ||
        fwrite(r.data(), sizeof(mpcr::StepRecords), 1, o) != 1)
      return 6;
    fclose(o);
    printf("%s npair=%d neq=%d\n", argv[a], m[0].npair, m[0].neq);
  }
  return 0;
}
