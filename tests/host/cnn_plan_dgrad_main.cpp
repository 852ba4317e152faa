// tests/host/cnn_plan_dgrad_main.cpp -- which form conv2's two gradient kernels take (csrc/kws_cnn_plan.h: dgrad2_fast, wgrad2_fast) as a
// plain host program: it reads one query per line from stdin,
//   kind nf fs C head_K B mprec det capturing
// builds the training plan and answers with one line of JSON, {"dgrad2_fast": ..., "wgrad2_fast": ..., "H1": ..., "W1": ...}.
// It holds no case table of its own; tests/test_conv2_dgrad_plan_host.py owns the cases.  A malformed query is answered with
// {"error": ...} and makes the exit status 1.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "kws_cnn_plan.h"

using namespace kws;

int main()
{
    int status = 0;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int kind, nf, fs, C, head_K, B, mprec, det, capturing;
        if (!(in >> kind >> nf >> fs >> C >> head_K >> B >> mprec >> det >> capturing)) {
            std::printf("{\"error\": \"malformed query\"}\n");
            status = 1;
            continue;
        }
        const CnnDesc m{kind, C, head_K, det, cnn_dims(nf, fs)};
        const CnnPlan p = plan_cnn(m, B, mprec, /*training=*/true, capturing != 0, /*wants_head_outputs=*/false, /*prepared=*/false);
        std::printf("{\"dgrad2_fast\": %s, \"wgrad2_fast\": %s, \"H1\": %d, \"W1\": %d}\n", p.dgrad2_fast ? "true" : "false",
                    p.wgrad2_fast ? "true" : "false", m.d.H1, m.d.W1);
    }
    return status;
}
