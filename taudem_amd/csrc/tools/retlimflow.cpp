// retlimflow -ang ang -wg wg -rc rc -qrl qrl   (flag surface of src/RetLimFlowmn.cpp:51-150)
#include "cli_common.hpp"

static void usage(const char* prog) {
    printf("Simple use:\n %s <basefilename>\n", prog);
    printf("General use:\n %s -ang <angfile> -wg <wgfile> -rc <rcfile> -qrl <qrlfile>\n", prog);
    printf("  <angfile>  D-infinity flow direction input\n");
    printf("  <wgfile>   weight (runoff excess) input\n");
    printf("  <rcfile>   retention capacity input\n");
    printf("  <qrlfile>  retention limited runoff output\n");
    printf("With the simple form the suffixes ang, wg, rc and qrl are inserted before the extension of <basefilename>.\n");
    exit(0);
}

int main(int argc, char** argv) {
    cli::take_gpus(argc, argv);
    std::string angfile, wgfile, rcfile, qrlfile;
    if (argc < 2) { printf("Error: use either the simple form or the form with explicit file names\n"); usage(argv[0]); }
    cli::Args a(argc, argv);
    while (a.more()) {
        if (a.is("-ang")) { if (!a.value(angfile)) usage(argv[0]); }
        else if (a.is("-wg")) { if (!a.value(wgfile)) usage(argv[0]); }
        else if (a.is("-rc")) { if (!a.value(rcfile)) usage(argv[0]); }
        else if (a.is("-qrl")) { if (!a.value(qrlfile)) usage(argv[0]); }
        else usage(argv[0]);
    }
    if (argc == 2) {
        angfile = cli::nameadd(argv[1], "ang"); rcfile = cli::nameadd(argv[1], "rc"); qrlfile = cli::nameadd(argv[1], "qrl"); wgfile = cli::nameadd(argv[1], "wg");
    }
    const int err = tdx_tool_retlimflow(angfile.c_str(), wgfile.c_str(), rcfile.c_str(), qrlfile.c_str());
    return cli::finish("Retention limited flow accumulation", err);
}
