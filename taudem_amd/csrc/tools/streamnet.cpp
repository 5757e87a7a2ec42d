// streamnet -fel fel -p p -ad8 ad8 -src src -ord ord -tree tree -coord coord -w w [-o outlets] [-lyrname n] [-lyrno i] [-sw] [-v] [-links host|device]
// (flag surface of src/streamnetmn.cpp:51-270), or streamnet <basefilename>.
// -net / -netlyr are recognised and refused before anything runs: the stream network layer is not written (every one of its fields follows from the
// tree and coord files).  The simple form writes the other four outputs and says so.  -links says where the links are built (host: the default);
// any other word ends the run with status 2 before anything is read.  Both write the same bytes.
#include "cli_common.hpp"

static void usage(const char* prog) {
    printf("Simple Usage:\n %s <basefilename>\n", prog);
    printf("Usage with specific file names:\n %s -p <pfile>\n", prog);
    printf("-fel <elevfile> -ad8 <ad8file> -src <srcfile>\n");
    printf("-ord <ordfile> -tree <treefile> -coord <coordfile>\n");
    printf("-w <wfile> [-o <outletfile>] [-sw]\n");
    printf("<basefilename> is the name of the base digital elevation model\n");
    printf("<pfile> is the D8 flow direction input file.\n");
    printf("<elevfile> is the pit filled or carved elevation input file.\n");
    printf("<ad8file> is the D8 contributing area input file.\n");
    printf("<srcfile> is the stream raster input file.\n");
    printf("<ordfile> is the stream order output file, <wfile> the watershed output file.\n");
    printf("<treefile> and <coordfile> are the network tree and coordinate output text files.\n");
    printf("The following are appended to the file names\n");
    printf("before the files are opened:\n");
    printf("fel, p, ad8, src (inputs); ord, w, tree.txt, coord.txt (outputs)\n");
    exit(0);
}

int main(int argc, char** argv) {
    cli::take_gpus(argc, argv);
    std::string pfile, srcfile, ordfile, ad8file, elevfile, wfile, outletsds, lyrname, netfile, netlyr, treefile, coordfile, linkswhere = "host";
    int uselayername = 0, lyrno = 0, verbose = 0;
    long ordert = 1, useoutlets = 0;
    if (argc < 2) {
        printf("Error: To run this program, use either the Simple Usage option or\n");
        printf("the Usage with Specific file names option\n");
        usage(argv[0]);
    }
    cli::Args a(argc, argv);
    while (a.more()) {
        if (a.is("-fel")) { if (!a.value(elevfile)) usage(argv[0]); }
        else if (a.is("-p")) { if (!a.value(pfile)) usage(argv[0]); }
        else if (a.is("-ad8")) { if (!a.value(ad8file)) usage(argv[0]); }
        else if (a.is("-src")) { if (!a.value(srcfile)) usage(argv[0]); }
        else if (a.is("-ord")) { if (!a.value(ordfile)) usage(argv[0]); }
        else if (a.is("-tree")) { if (!a.value(treefile)) usage(argv[0]); }
        else if (a.is("-coord")) { if (!a.value(coordfile)) usage(argv[0]); }
        else if (a.is("-o")) { if (!a.value(outletsds)) usage(argv[0]); useoutlets = 1; }
        else if (a.is("-lyrno")) { if (!a.value(lyrno)) usage(argv[0]); }
        else if (a.is("-lyrname")) { if (!a.value(lyrname)) usage(argv[0]); uselayername = 1; }
        else if (a.is("-w")) { if (!a.value(wfile)) usage(argv[0]); }
        else if (a.is("-net")) { if (!a.value(netfile)) usage(argv[0]); }
        else if (a.is("-netlyr")) { if (!a.value(netlyr)) usage(argv[0]); }
        else if (a.is("-links")) { if (!a.value(linkswhere)) usage(argv[0]); }
        else if (a.is("-sw")) { a.flag(); ordert = 0; }
        else if (a.is("-v")) { a.flag(); verbose = 1; }
        else usage(argv[0]);
    }
    // (the layer itself exists one level down: tdx_streamnet_net_write makes it from the links of tdx_streamnet, and catchoutlets takes -tree / -coord)
    if (!netfile.empty() || !netlyr.empty()) {
        fprintf(stderr, "streamnet: -net / -netlyr are not supported: the stream network layer is not written; its fields follow from the -tree and -coord files\n");
        return 2;
    }
    if (linkswhere != "host" && linkswhere != "device") {
        fprintf(stderr, "streamnet: -links takes host or device, not %s\n", linkswhere.c_str());
        return 2;
    }
    tdx_tool_set_streamnet_links(linkswhere == "device" ? 1 : 0);
    if (argc == 2) {
        const std::string base = argv[1];
        elevfile = cli::nameadd(base, "fel"); pfile = cli::nameadd(base, "p"); ad8file = cli::nameadd(base, "ad8"); srcfile = cli::nameadd(base, "src");
        ordfile = cli::nameadd(base, "ord"); treefile = cli::nameadd(base, "tree.txt"); coordfile = cli::nameadd(base, "coord.txt"); wfile = cli::nameadd(base, "w");
        fprintf(stderr, "streamnet: the stream network file is not written\n");
    }
    const int err = tdx_tool_streamnet(pfile.c_str(), srcfile.c_str(), ordfile.c_str(), ad8file.c_str(), elevfile.c_str(), treefile.c_str(), coordfile.c_str(),
                                       outletsds.c_str(), lyrname.c_str(), uselayername, lyrno, wfile.c_str(), "", "", useoutlets, ordert, verbose);
    if (err == 4) { fflush(stdout); return 4; }   // MPI_Abort(MCW, 4): a raster that does not match src
    return cli::finish("StreamNet", err);
}
